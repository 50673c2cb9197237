// lookup.hip - differentiable field lookups at given points (reference models/tensorf_keyframe.py:233-310 under autograd):
//   nvfi_density_grad   the adjoint of compute_densityfeature (the forward IS nvfi_density_at): feat = sum_c prod_i space_i[c] prod_i time_i[c]
//   nvfi_appfeat_at     compute_appfeature: feat = basis_mat (prod_i space_i prod_i time_i)
//   nvfi_appfeat_grad   its adjoint
// The time coordinate is per point and may be fractional or out of range: all six planes of a family take four taps of
// F.grid_sample(align_corners=True, padding_mode="zeros").  The tap set is common.h's bl_setup_xy on the fp32 coordinates - cell, masks and the
// four weights - so the value and both gradients see the same cell as nvfi_density_at.  Nothing is stashed: the backward reads the taps again,
// forms each plane's share as upstream x the product of the other five bilinear values and adds it to the four texels; the coordinate
// gradient is ATen's grid_sampler_2d_backward (the difference of the in-range taps times (W - 1) / 2, (H - 1) / 2, and (K - 1) / 2 for t').
// Lane layout as in charloss.hip - one wave per point in a grid-stride loop, lanes are CHANNELS, per-point quantities are wave-uniform:
//   density (24 channels)  lane = 2 * channel + x-tap: one load / atomic instruction covers two neighbouring texels (192 B); 12 per point = 2304 B
//   appearance (48)        lane = channel: one texel per instruction (192 B); 24 per point = 4608 B
// basis_mat (app_dim x 48) sits in LDS with an odd row stride; per point one lane per channel forms W^T g_feat, and dW = sum g_feat prod^T is
// kept in registers per wave (lane = column), reduced per workgroup in LDS, and only then added to global memory.
// g_xyzt and feat are plain stores, folded over the lanes with a fixed butterfly: they repeat bit for bit.  The plane and basis_mat gradients
// are float atomics into buffers the caller zeroed: they do NOT repeat bit for bit and are not covered by NVFI_DETERMINISTIC.
// No workspace, no clearing, no allocation, no host wait: every call is a single launch on `stream` and can be captured in a hipGraph.
#include <string.h>
#include "common.h"
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

__device__ __forceinline__ float look_uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float look_bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// the six tap sets of a point (wave-uniform).  A plane none of whose taps is in range gets zero weights: a non-finite coordinate leaves NaN in
// them, and the coordinate gradient multiplies weights with (zeroed) taps.  A plane with a tap in range has finite weights on both axes.
__device__ __forceinline__ void look_setups(const nvfi_field_desc& f, const float* q, Bl* b) {
    const float4 p = ld4(q);
    plane_setups(f, look_uni(p.x), look_uni(p.y), look_uni(p.z), look_uni(p.w), b);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!(b[i].m0 || b[i].m1 || b[i].m2 || b[i].m3)) { b[i].w = 0.f; b[i].e = 0.f; b[i].n = 0.f; b[i].s = 0.f; }
}
// upstream x the product of the other five values
__device__ __forceinline__ void other_five(const float* val, float g, float* o) {
    float L[6], R[6];
    L[0] = g;
#pragma unroll
    for (int p = 1; p < 6; ++p) L[p] = L[p - 1] * val[p - 1];
    R[5] = 1.f;
#pragma unroll
    for (int p = 4; p >= 0; --p) R[p] = R[p + 1] * val[p + 1];
#pragma unroll
    for (int p = 0; p < 6; ++p) o[p] = L[p] * R[p];
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

// ---------------------------------------------------------------- density: lane = 2 * channel + x-tap
__global__ __launch_bounds__(256) void k_lookup_density_bwd(LookArgs a) {
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * nwv + (threadIdx.x >> 6)), wtot = (int64_t)gridDim.x * nwv;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane >> 1 : 0, dx0 = lane & 1;
    const float* pl[6]; float* gp[6];
#pragma unroll
    for (int p = 0; p < 3; ++p) { pl[p] = f.dps[p]; pl[3 + p] = f.dpt[p]; gp[p] = a.g.dps[p]; gp[3 + p] = a.g.dpt[p]; }
#pragma unroll 1
    for (int64_t n = wave0; n < a.N; n += wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        const float g = look_uni(a.gf[n]);
        float val[6], dx[6], dy[6], wx[6];
        size_t o0[6], o1[6];
        bool my0[6], my1[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            my0[p] = lane_on && (dx0 ? b[p].m1 : b[p].m0); my1[p] = lane_on && (dx0 ? b[p].m3 : b[p].m2);
            wx[p] = dx0 ? b[p].w : b[p].e;
            o0[p] = my0[p] ? (size_t)(b[p].base + dx0) * 24 + ch : 0;                  // a masked tap reads texel 0 and is zeroed by a select
            o1[p] = my1[p] ? (size_t)(b[p].base + dx0 + b[p].W) * 24 + ch : 0;
        }
        float v0[6], v1[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) { v0[p] = pl[p][o0[p]]; v1[p] = pl[p][o1[p]]; }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            v0[p] = my0[p] ? v0[p] : 0.f; v1[p] = my1[p] ? v1[p] : 0.f;
            const float part = v0[p] * (wx[p] * b[p].s) + v1[p] * (wx[p] * b[p].n);
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
        for (int p = 0; p < 6; ++p) {
            if (!gp[p]) continue;
            if (my0[p]) atomicAdd(gp[p] + o0[p], (wx[p] * b[p].s) * o[p]);
            if (my1[p]) atomicAdd(gp[p] + o1[p], (wx[p] * b[p].n) * o[p]);
        }
    }
}

// ---------------------------------------------------------------- appearance: lane = channel (48 of 64 lanes)
struct AppTaps { size_t o[4]; bool m[4]; };
__device__ __forceinline__ void app_taps(const Bl& b, int ch, bool lane_on, AppTaps& t) {
    t.m[0] = lane_on && b.m0; t.m[1] = lane_on && b.m1; t.m[2] = lane_on && b.m2; t.m[3] = lane_on && b.m3;
    t.o[0] = t.m[0] ? (size_t)b.base * 48 + ch : 0;
    t.o[1] = t.m[1] ? (size_t)(b.base + 1) * 48 + ch : 0;
    t.o[2] = t.m[2] ? (size_t)(b.base + b.W) * 48 + ch : 0;
    t.o[3] = t.m[3] ? (size_t)(b.base + b.W + 1) * 48 + ch : 0;
}
// the six bilinear values of this lane's channel (0 in lanes >= 48); v keeps the zero-padded taps
__device__ __forceinline__ void app_vals(const float* const* pl, const Bl* b, const AppTaps* t, float (*v)[4], float* val) {
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p][k] = pl[p][t[p].o[k]];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p][k] = t[p].m[k] ? v[p][k] : 0.f;
        val[p] = v[p][0] * (b[p].e * b[p].s) + v[p][1] * (b[p].w * b[p].s) + v[p][2] * (b[p].e * b[p].n) + v[p][3] * (b[p].w * b[p].n);
    }
}
__device__ __forceinline__ float prod6(const float* v) { return ((v[0] * v[1]) * v[2]) * ((v[3] * v[4]) * v[5]); }

#define LK_WSTRIDE 49      // LDS row stride of basis_mat: odd, so lanes that read a column (row = lane) hit 32 different banks
__device__ __forceinline__ void stage_basis(const nvfi_field_desc& f, float* Wl, float* red) {
    for (int k = threadIdx.x; k < 32 * 48; k += blockDim.x) {
        const int j = k / 48, c = k - 48 * j;
        Wl[j * LK_WSTRIDE + c] = j < f.app_dim ? f.basis[k] : 0.f;      // rows >= app_dim zero
        if (red) red[k] = 0.f;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_lookup_app_fwd(LookArgs a) {
    __shared__ float Wl[32 * LK_WSTRIDE];
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * nwv + (threadIdx.x >> 6)), wtot = (int64_t)gridDim.x * nwv;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane : 0, jrow = lane & 31;
    const int app_dim = f.app_dim;
    stage_basis(f, Wl, nullptr);
    const float* pl[6];
#pragma unroll
    for (int p = 0; p < 3; ++p) { pl[p] = f.aps[p]; pl[3 + p] = f.apt[p]; }
#pragma unroll 1
    for (int64_t n = wave0; n < a.N; n += wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        AppTaps t[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) app_taps(b[p], ch, lane_on, t[p]);
        float v[6][4], val[6];
        app_vals(pl, b, t, v, val);
        const float pr = prod6(val);
        float y = 0.f;                                                     // lane j < app_dim: (W prod)_j
#pragma unroll 8
        for (int c = 0; c < 48; ++c) y += Wl[jrow * LK_WSTRIDE + c] * look_bcast(pr, c);
        if (lane < app_dim) a.feat[n * app_dim + lane] = y;
    }
}

__global__ __launch_bounds__(256) void k_lookup_app_bwd(LookArgs a) {
    __shared__ float Wl[32 * LK_WSTRIDE];      // basis_mat
    __shared__ float red[32 * 48];             // dW of the workgroup
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
    const int64_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * nwv + (threadIdx.x >> 6)), wtot = (int64_t)gridDim.x * nwv;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane : 0;
    const int app_dim = f.app_dim;
    stage_basis(f, Wl, red);
    const float* pl[6]; float* gp[6];
#pragma unroll
    for (int p = 0; p < 3; ++p) { pl[p] = f.aps[p]; pl[3 + p] = f.apt[p]; gp[p] = a.g.aps[p]; gp[3 + p] = a.g.apt[p]; }
    const bool want_w = a.g.basis != nullptr;
    float accW[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) accW[j] = 0.f;
#pragma unroll 1
    for (int64_t n = wave0; n < a.N; n += wtot) {
        Bl b[6];
        look_setups(f, a.q + 4 * n, b);
        AppTaps t[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) app_taps(b[p], ch, lane_on, t[p]);
        const float gfv = lane < app_dim ? a.gf[n * app_dim + lane] : 0.f;  // lane j: g_feat[j]
        float v[6][4], val[6];
        app_vals(pl, b, t, v, val);
        const float pr = prod6(val);
        float gl = 0.f;                                                     // lane c < 48: (W^T g_feat)_c
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float gj = look_bcast(gfv, j);
            gl += Wl[j * LK_WSTRIDE + ch] * gj;
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
        for (int p = 0; p < 6; ++p) {
            if (!gp[p]) continue;
            if (t[p].m[0]) atomicAdd(gp[p] + t[p].o[0], (b[p].e * b[p].s) * o[p]);
            if (t[p].m[1]) atomicAdd(gp[p] + t[p].o[1], (b[p].w * b[p].s) * o[p]);
            if (t[p].m[2]) atomicAdd(gp[p] + t[p].o[2], (b[p].e * b[p].n) * o[p]);
            if (t[p].m[3]) atomicAdd(gp[p] + t[p].o[3], (b[p].w * b[p].n) * o[p]);
        }
    }
    if (want_w) {
        if (lane_on) {
#pragma unroll
            for (int j = 0; j < 32; ++j)
                if (accW[j] != 0.f) atomicAdd(&red[j * 48 + ch], accW[j]);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < app_dim * 48; k += blockDim.x)
            if (red[k] != 0.f) atomicAdd(a.g.basis + k, red[k]);
    }
}

// ---------------------------------------------------------------- host
static const int64_t LOOKUP_N_MAX = (1ll << 31) - 256;       // nvfi_density_at's limit
// a wave walks the points with a grid stride: at least four points per wave, at most `per_cu` workgroups per CU
static unsigned lookup_grid(int64_t N, int per_cu) {
    const int64_t want = (N + 15) / 16, cap = (int64_t)per_cu * device_cu_count();
    return (unsigned)(want < cap ? want : cap);
}
static int lookup_check(const char* name, const nvfi_field_desc* f, int64_t N, const float* xyzt, const void* other) {
    if (check_desc(f)) return 2;
    if (N <= 0) return -1;
    if (N >= LOOKUP_N_MAX) return nvfi_fail(2, "%s: N too large for one call; chunk the points", name);
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
    hipLaunchKernelGGL(k_lookup_density_bwd, dim3(lookup_grid(N, 8)), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCHCK();
    return 0;
}
extern "C" int nvfi_appfeat_at(const nvfi_field_desc* f, int64_t N, const float* xyzt, float* feat, void* stream) {
    if (const int rc = lookup_check("nvfi_appfeat_at", f, N, xyzt, feat)) return rc < 0 ? 0 : rc;
    LookArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.N = N; a.q = xyzt; a.feat = feat;
    hipLaunchKernelGGL(k_lookup_app_fwd, dim3(lookup_grid(N, 8)), dim3(256), 0, (hipStream_t)stream, a);
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
    // at most four workgroups per CU, so that the per-workgroup flush of dW stays a small share
    hipLaunchKernelGGL(k_lookup_app_bwd, dim3(lookup_grid(N, 4)), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCHCK();
    return 0;
}
