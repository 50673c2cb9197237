// lookup.hip - differentiable field lookups at given points (reference models/tensorf_keyframe.py:233-310 under autograd):
//   nvfi_density_grad   the adjoint of compute_densityfeature (the forward IS nvfi_density_at): feat = sum_c prod_i space_i[c] prod_i time_i[c]
//   nvfi_appfeat_at     compute_appfeature: feat = basis_mat (prod_i space_i prod_i time_i)
//   nvfi_appfeat_grad   its adjoint
// The time coordinate is per point and may be fractional or out of range: all six planes of a family take four taps of
// F.grid_sample(align_corners=True, padding_mode="zeros").  The tap set is common.h's bl_setup_xy on the fp32 coordinates - cell, masks and the
// four weights - so the value and both gradients see the same cell as nvfi_density_at.  Nothing is stashed: the backward reads the taps again,
// forms each plane's share as upstream x the product of the other five bilinear values and adds it to the four texels; the coordinate
// gradient is ATen's grid_sampler_2d_backward (the difference of the in-range taps times (W - 1) / 2, (H - 1) / 2, and (K - 1) / 2 for t').
// One wave per point, lanes are channels, per-point quantities are wave-uniform (pointwave.h: the lane layouts, the tap sets, basis_mat in LDS, the
// dW flush).  Per point the density adjoint issues 12 tap instructions = 2304 B, the appearance kernels 24 = 4608 B.
// g_xyzt and feat are plain stores, folded over the lanes with a fixed butterfly: they repeat bit for bit.  The plane and basis_mat gradients
// are float atomics into buffers the caller zeroed: they do NOT repeat bit for bit and are not covered by NVFI_DETERMINISTIC.
// No workspace, no clearing, no allocation, no host wait: every call is a single launch on `stream` and can be captured in a hipGraph.
#include <string.h>
#include "pointwave.h"
#include "render.h"

struct LookArgs {
    nvfi_field_desc f;
    nvfi_grads g;          // density: dps / dpt; appearance: aps / apt / basis; NULL members are skipped
    int64_t N;
    const float* q;        // (N,4) normalised x, y, z, t'
    const float* gf;       // upstream gradient: (N) density, (N, app_dim) appearance
    float* gq;             // (N,4) coordinate gradient, overwritten; or NULL
    float* feat;           // (N, app_dim): the appearance forward
};

// the six tap sets of a point (wave-uniform).  A plane none of whose taps is in range gets zero weights: a non-finite coordinate leaves NaN in
// them, and the coordinate gradient multiplies weights with (zeroed) taps.  A plane with a tap in range has finite weights on both axes.
__device__ __forceinline__ void look_setups(const nvfi_field_desc& f, const float* q, Bl* b) {
    const float4 p = ld4(q);
    plane_setups(f, uni(p.x), uni(p.y), uni(p.z), uni(p.w), b);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!(b[i].m0 || b[i].m1 || b[i].m2 || b[i].m3)) { b[i].w = 0.f; b[i].e = 0.f; b[i].n = 0.f; b[i].s = 0.f; }
}
// routing of the per-plane texel-coordinate gradients (gx[p], gy[p], p = space 0..2, time 3..5) to x, y, z, t' (matModeSpace / matModeTime),
// summed over the wave and scaled by (G - 1) / 2 resp. (K - 1) / 2; lane l < 4 stores component l
__device__ __forceinline__ void coord_store(const nvfi_field_desc& f, const float* gx, const float* gy, int lane, float* out) {
    const float ax = wave_sum((gx[0] + gx[1]) + gx[5]);
    const float ay = wave_sum((gy[0] + gx[2]) + gx[4]);
    const float az = wave_sum((gy[1] + gy[2]) + gx[3]);
    const float at = wave_sum((gy[3] + gy[4]) + gy[5]);
    const int gx0 = f.G[0], gx1 = f.G[1], gx2 = f.G[2], k = f.K;
    const float rx = ax * ((float)(gx0 - 1) / 2.f), ry = ay * ((float)(gx1 - 1) / 2.f), rz = az * ((float)(gx2 - 1) / 2.f), rt = at * ((float)(k - 1) / 2.f);
    float r = rt;
    r = lane == 2 ? rz : r; r = lane == 1 ? ry : r; r = lane == 0 ? rx : r;
    if (lane < 4) out[lane] = r;
}

// Loads here are UNCONDITIONAL and then selected (the taps of all six planes are in flight together): a masked tap reads texel 0, so its offset -
// and ch in the idle lanes - is clamped to 0 before the load.  (charloss.hip loads under the mask and never clamps.)
template <int NT> __device__ __forceinline__ void clamp_taps(LaneTaps<NT>& t) {
#pragma unroll
    for (int k = 0; k < NT; ++k) t.o[k] = t.m[k] ? t.o[k] : 0;
}

// ---------------------------------------------------------------- density
__global__ __launch_bounds__(256) void k_lookup_density_bwd(LookArgs a) {
    const nvfi_field_desc& f = a.f;
    const PointWalk w;
    const int lane = w.lane;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane >> 1 : 0, dx0 = lane & 1;
    const float* pl[6]; float* gp[6];
    family_planes(f.dps, f.dpt, pl);
    family_planes(a.g.dps, a.g.dpt, gp);
#pragma unroll 1
    for (int64_t n = w.wave0; n < a.N; n += w.wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        const float g = uni(a.gf[n]);
        float val[6], dx[6], dy[6], wx[6];
        LaneTaps<2> t[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) { density_taps(b[p], ch, dx0, lane_on, t[p], wx[p]); clamp_taps(t[p]); }
        float v0[6], v1[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) { v0[p] = pl[p][t[p].o[0]]; v1[p] = pl[p][t[p].o[1]]; }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            v0[p] = t[p].m[0] ? v0[p] : 0.f; v1[p] = t[p].m[1] ? v1[p] : 0.f;
            const float part = v0[p] * t[p].w[0] + v1[p] * t[p].w[1];
            val[p] = part + __shfl_xor(part, 1);                                        // both lanes of a pair: the channel's bilinear value
            const float row = v0[p] * b[p].s + v1[p] * b[p].n;
            dx[p] = dx0 ? row : -row;                                                   // d value / d texel-x: this lane's x-tap
            dy[p] = (v1[p] - v0[p]) * wx[p];
        }
        float o[6];
        other_five(val, g, o);
        if (a.gq) {
#pragma unroll
            for (int p = 0; p < 6; ++p) { dx[p] *= o[p]; dy[p] *= o[p]; }
            coord_store(f, dx, dy, lane, a.gq + 4 * n);
        }
#pragma unroll
        for (int p = 0; p < 6; ++p)
            if (gp[p]) scatter_taps(gp[p], t[p], o[p]);
    }
}

// ---------------------------------------------------------------- appearance
// the six bilinear values of this lane's channel (0 in lanes >= 48); v keeps the zero-padded taps
__device__ __forceinline__ void app_vals(const float* const* pl, const Bl* b, int ch, bool lane_on, LaneTaps<4>* t, float (*v)[4], float* val) {
#pragma unroll
    for (int p = 0; p < 6; ++p) { app_taps(b[p], ch, lane_on, t[p]); clamp_taps(t[p]); }
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p][k] = pl[p][t[p].o[k]];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p][k] = t[p].m[k] ? v[p][k] : 0.f;
        val[p] = v[p][0] * t[p].w[0] + v[p][1] * t[p].w[1] + v[p][2] * t[p].w[2] + v[p][3] * t[p].w[3];
    }
}

__global__ __launch_bounds__(256) void k_lookup_app_fwd(LookArgs a) {
    __shared__ float Wl[32 * PW_WSTRIDE];
    const nvfi_field_desc& f = a.f;
    const PointWalk w;
    const int lane = w.lane;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane : 0, jrow = lane & 31;
    const int app_dim = f.app_dim;
    stage_basis(f, Wl, nullptr);
    const float* pl[6];
    family_planes(f.aps, f.apt, pl);
#pragma unroll 1
    for (int64_t n = w.wave0; n < a.N; n += w.wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        LaneTaps<4> t[6];
        float v[6][4], val[6];
        app_vals(pl, b, ch, lane_on, t, v, val);
        const float pr = prod6(val);
        float y = 0.f;                                                     // lane j < app_dim: (W prod)_j
#pragma unroll 8
        for (int c = 0; c < 48; ++c) y += Wl[jrow * PW_WSTRIDE + c] * lane_bcast(pr, c);
        if (lane < app_dim) a.feat[n * app_dim + lane] = y;
    }
}

__global__ __launch_bounds__(256) void k_lookup_app_bwd(LookArgs a) {
    __shared__ float Wl[32 * PW_WSTRIDE];      // basis_mat
    __shared__ float red[32 * 48];             // dW of the workgroup
    const nvfi_field_desc& f = a.f;
    const PointWalk w;
    const int lane = w.lane;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane : 0;
    const int app_dim = f.app_dim;
    stage_basis(f, Wl, red);
    const float* pl[6]; float* gp[6];
    family_planes(f.aps, f.apt, pl);
    family_planes(a.g.aps, a.g.apt, gp);
    const bool want_w = a.g.basis != nullptr;
    float accW[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) accW[j] = 0.f;
#pragma unroll 1
    for (int64_t n = w.wave0; n < a.N; n += w.wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        const float gfv = lane < app_dim ? a.gf[n * app_dim + lane] : 0.f;  // lane j: g_feat[j]
        LaneTaps<4> t[6];
        float v[6][4], val[6];
        app_vals(pl, b, ch, lane_on, t, v, val);
        const float pr = prod6(val);
        float gl = 0.f;                                                     // lane c < 48: (W^T g_feat)_c
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float gj = lane_bcast(gfv, j);
            gl += Wl[j * PW_WSTRIDE + ch] * gj;
            if (want_w) accW[j] += gj * pr;
        }
        if (!lane_on) gl = 0.f;
        float o[6];
        other_five(val, gl, o);
        if (a.gq) {
            float dx[6], dy[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                dx[p] = ((v[p][1] - v[p][0]) * b[p].s + (v[p][3] - v[p][2]) * b[p].n) * o[p];
                dy[p] = ((v[p][2] - v[p][0]) * b[p].e + (v[p][3] - v[p][1]) * b[p].w) * o[p];
            }
            coord_store(f, dx, dy, lane, a.gq + 4 * n);
        }
#pragma unroll
        for (int p = 0; p < 6; ++p)
            if (gp[p]) scatter_taps(gp[p], t[p], o[p]);
    }
    if (want_w) flush_dw(accW, red, ch, lane_on, app_dim, 1.f, a.g.basis);
}

// ---------------------------------------------------------------- host
static int lookup_check(const char* name, const nvfi_field_desc* f, int64_t N, const float* xyzt, const void* other) {
    if (check_desc(f)) return 2;
    if (N <= 0) return -1;
    if (N >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "%s: N too large for one call; chunk the points", name);
    if (!xyzt || !other) return nvfi_fail(2, "%s: a NULL input", name);
    return 0;
}

extern "C" int nvfi_density_grad(const nvfi_field_desc* f, int64_t N, const float* xyzt, const float* g_feat, float* g_xyzt,
                                 const nvfi_grads* grads, void* stream) {
    if (const int rc = lookup_check("nvfi_density_grad", f, N, xyzt, g_feat)) return rc < 0 ? 0 : rc;
    LookArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.N = N; a.q = xyzt; a.gf = g_feat; a.gq = g_xyzt;
    bool any = g_xyzt != nullptr;
    if (grads)
        for (int i = 0; i < 3; ++i) { a.g.dps[i] = grads->dps[i]; a.g.dpt[i] = grads->dpt[i]; any = any || grads->dps[i] || grads->dpt[i]; }
    if (!any) return 0;
    hipLaunchKernelGGL(k_lookup_density_bwd, dim3(point_grid(N, 8)), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCHCK();
    return 0;
}
extern "C" int nvfi_appfeat_at(const nvfi_field_desc* f, int64_t N, const float* xyzt, float* feat, void* stream) {
    if (const int rc = lookup_check("nvfi_appfeat_at", f, N, xyzt, feat)) return rc < 0 ? 0 : rc;
    LookArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.N = N; a.q = xyzt; a.feat = feat;
    hipLaunchKernelGGL(k_lookup_app_fwd, dim3(point_grid(N, 8)), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCHCK();
    return 0;
}
extern "C" int nvfi_appfeat_grad(const nvfi_field_desc* f, int64_t N, const float* xyzt, const float* g_feat, float* g_xyzt,
                                 const nvfi_grads* grads, void* stream) {
    if (const int rc = lookup_check("nvfi_appfeat_grad", f, N, xyzt, g_feat)) return rc < 0 ? 0 : rc;
    LookArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.N = N; a.q = xyzt; a.gf = g_feat; a.gq = g_xyzt;
    bool any = g_xyzt != nullptr;
    if (grads) {
        for (int i = 0; i < 3; ++i) { a.g.aps[i] = grads->aps[i]; a.g.apt[i] = grads->apt[i]; any = any || grads->aps[i] || grads->apt[i]; }
        a.g.basis = grads->basis; any = any || grads->basis;
    }
    if (!any) return 0;
    hipLaunchKernelGGL(k_lookup_app_bwd, dim3(point_grid(N, 4)), dim3(256), 0, (hipStream_t)stream, a);      // (flushes dW per workgroup)
    LAUNCHCK();
    return 0;
}
