// charloss.hip - characteristic loss (reference models/tensorf_keyframe.py:552-573): keyframe transport consistency of the factor planes.
//   loss = mean_N (d_t - d_0)^2 + mean_{N x app_dim} (a_t - a_0)^2
//   d_t / a_t: compute_densityfeature / compute_appfeature at (x, keyframe row k);  d_0 / a_0: the same at (x0, row 0), x0 = integrate_pos(x, t_k, 0)
// Value and gradients (twelve planes + basis_mat) come out of ONE pass per plane family: no gradient depends on the loss total, so every
// contribution is scaled by a weight known before the launch.  The time is uniform per call and sits ON a keyframe, so the time coordinate of
// both lookups is an integer row (a host scalar): the time planes are read with the two x-taps of that row, the space planes with four taps.
// One wave per point, lanes are channels (pointwave.h: the lane layouts, the tap sets, basis_mat in LDS, the dW flush); the loss sums follow reduce.h.
// basis_mat has no bias: a_t - a_0 = W (g_t - g_0).  Per point one lane per output row forms y = W dg, one lane per channel forms W^T y, and
// dW = sum y dg^T.  Plane gradients are float atomics (the call is not covered by NVFI_DETERMINISTIC).
#include <string.h>
#include "reduce.h"
#include "pointwave.h"

struct CharArgs {
    nvfi_field_desc f;
    nvfi_grads g;          // all NULL: value only
    int64_t N;
    const float* x;        // (N,3) normalised points at the keyframe time
    const float* x0;       // (N,3) the points advected back to keyframe 0
    int row;               // keyframe row k of the t side (the 0 side reads row 0)
    float s_d, s_a;        // weight * 2 / N,  weight * 2 / (app_dim * N)
    double* acc;           // [2] sum (d_t - d_0)^2, sum |W dg|^2
};

// The tap sets of a point are formed HERE, not by common.h's plane_setups as in lookup.hip: the time coordinate is the integer keyframe row, and
// DESIGN 4.15 measured 4.27 x the allowed error with the fp32 setup.
// One axis of a tap set.  The texel coordinate is formed in double and only the two weights are rounded to fp32: an fp32 coordinate
// carries half an ulp of a number up to W into the weights (5e-7 absolute at W = 16), which is as large as the whole error the loss may
// show at a single point.  The points themselves are fp32 data.  The setup is wave-uniform, so the doubles cost a few scalar-like ops per point.
__device__ __forceinline__ int bl_axis(float g, int W, float& w, float& e) {
    const double x = ((double)g + 1.0) * ((double)(W - 1) * 0.5);
    double xf = floor(x);
    const double wd = x - xf;
    w = (float)wd; e = (float)(1.0 - wd);
    xf = fmin(fmax(xf, -4.0), (double)W + 2.0);
    if (!(xf == xf)) xf = -4.0;
    return (int)xf;
}
// the four taps of a space plane: grid_sample(align_corners=True, zeros), the tap set of common.h's bl_setup
__device__ __forceinline__ void bl_plane(float gx, float gy, int W, int H, Bl& b) {
    const int x0 = bl_axis(gx, W, b.w, b.e), y0 = bl_axis(gy, H, b.n, b.s);
    const bool xi0 = x0 >= 0 && x0 < W, xi1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yi0 = y0 >= 0 && y0 < H, yi1 = y0 + 1 >= 0 && y0 + 1 < H;
    b.m0 = xi0 && yi0; b.m1 = xi1 && yi0; b.m2 = xi0 && yi1; b.m3 = xi1 && yi1;
    b.base = y0 * W + x0; b.W = W;
}
// the two x-taps of an integer time row: the same lookup whose y coordinate lands on `row`
__device__ __forceinline__ void bl_row(float g, int W, int row, Bl& b) {
    const int x0 = bl_axis(g, W, b.w, b.e);
    b.n = 0.f; b.s = 1.f;
    b.m0 = x0 >= 0 && x0 < W; b.m1 = x0 + 1 >= 0 && x0 + 1 < W; b.m2 = false; b.m3 = false;
    b.base = row * W + x0; b.W = W;
}
__device__ __forceinline__ void char_setups(const nvfi_field_desc& f, const float* p, int row, Bl* b) {
    const float x = uni(p[0]), y = uni(p[1]), z = uni(p[2]);
    bl_plane(x, y, f.G[0], f.G[1], b[0]);
    bl_plane(x, z, f.G[0], f.G[2], b[1]);
    bl_plane(y, z, f.G[1], f.G[2], b[2]);
    bl_row(z, f.G[2], row, b[3]);
    bl_row(y, f.G[1], row, b[4]);
    bl_row(x, f.G[0], row, b[5]);
}

// ---- density layout: both lanes of a pair end up with the channel's bilinear value.  Loads under the mask (ch is not clamped in lanes >= 48)
__device__ __forceinline__ void pair_vals(const float* const* pl, const Bl* b, int ch, int dx0, bool lane_on, LaneTaps<2>* t, float* val) {
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        float wx;
        density_taps(b[p], ch, dx0, lane_on, t[p], wx);
        const float v0 = t[p].m[0] ? pl[p][t[p].o[0]] : 0.f, v1 = t[p].m[1] ? pl[p][t[p].o[1]] : 0.f;
        const float part = (t[p].m[0] ? v0 * t[p].w[0] : 0.f) + (t[p].m[1] ? v1 * t[p].w[1] : 0.f);
        val[p] = part + __shfl_xor(part, 1);
    }
}
// g x the product of the other five values into the lane's texels of every plane that has a gradient buffer
template <int NT> __device__ __forceinline__ void char_scatter(float* const* gp, const LaneTaps<NT>* t, const float* val, float g) {
    float o[6];
    other_five(val, g, o);
#pragma unroll
    for (int p = 0; p < 6; ++p)
        if (gp[p]) scatter_taps(gp[p], t[p], o[p]);
}

__global__ __launch_bounds__(256) void k_char_density(CharArgs a) {
    const nvfi_field_desc& f = a.f;
    const PointWalk w;
    const int lane = w.lane, ch = lane >> 1, dx0 = lane & 1;
    const bool lane_on = lane < 48;
    const float* pl[6]; float* gp[6];
    family_planes(f.dps, f.dpt, pl);
    family_planes(a.g.dps, a.g.dpt, gp);
    double lsum = 0.0;
#pragma unroll 1
    for (int64_t n = w.wave0; n < a.N; n += w.wtot) {
        Bl bt[6], b0[6];
        char_setups(f, a.x + 3 * n, a.row, bt);
        char_setups(f, a.x0 + 3 * n, 0, b0);
        LaneTaps<2> tt[6], t0[6];
        float vt[6], v0[6];
        pair_vals(pl, bt, ch, dx0, lane_on, tt, vt);
        pair_vals(pl, b0, ch, dx0, lane_on, t0, v0);
        const float diff = wave_sum((lane_on && !dx0) ? prod6(vt) - prod6(v0) : 0.f);      // d_t - d_0, the same in every lane
        lsum += (double)diff * (double)diff;
        const float g = a.s_d * diff;
        char_scatter(gp, tt, vt, g);
        char_scatter(gp, t0, v0, -g);
    }
    if (lane == 0 && lsum != 0.0) atomicAdd(a.acc, lsum);
}

// ---- appearance layout
// returns the channel's product of the six bilinear values in double (the value path: g_t - g_0 cancels, and an fp32 product would hand the
// cancellation 3e-7 of each side) - its own weights in double, not the taps' fp32 ones; val[] keeps the six values in fp32 for the gradient's
// other-five products.  Loads under the mask
__device__ __forceinline__ double full_vals(const float* const* pl, const Bl* b, int ch, bool lane_on, LaneTaps<4>* t, float* val) {
    double prod = 1.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        app_taps(b[p], ch, lane_on, t[p]);
        const bool* m = t[p].m;
        const float v0 = m[0] ? pl[p][t[p].o[0]] : 0.f, v1 = m[1] ? pl[p][t[p].o[1]] : 0.f, v2 = m[2] ? pl[p][t[p].o[2]] : 0.f, v3 = m[3] ? pl[p][t[p].o[3]] : 0.f;
        const double e = b[p].e, w = b[p].w, n = b[p].n, s = b[p].s;
        const double v = (m[0] ? (double)v0 * (e * s) : 0.0) + (m[1] ? (double)v1 * (w * s) : 0.0) + (m[2] ? (double)v2 * (e * n) : 0.0) +
                         (m[3] ? (double)v3 * (w * n) : 0.0);
        val[p] = (float)v;
        prod *= v;
    }
    return lane_on ? prod : 0.0;
}

__global__ __launch_bounds__(256) void k_char_app(CharArgs a) {
    __shared__ float Wl[32 * PW_WSTRIDE];      // basis_mat
    __shared__ float red[32 * 48];             // dW of the workgroup
    const nvfi_field_desc& f = a.f;
    const PointWalk w;
    const int lane = w.lane;
    const bool lane_on = lane < 48;
    const int ch = lane_on ? lane : 0, jrow = lane & 31;
    stage_basis(f, Wl, red);
    const float* pl[6]; float* gp[6];
    family_planes(f.aps, f.apt, pl);
    family_planes(a.g.aps, a.g.apt, gp);
    const bool want_w = a.g.basis != nullptr;
    float accW[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) accW[j] = 0.f;
    double lsum = 0.0;
#pragma unroll 1
    for (int64_t n = w.wave0; n < a.N; n += w.wtot) {
        Bl bt[6], b0[6];
        char_setups(f, a.x + 3 * n, a.row, bt);
        char_setups(f, a.x0 + 3 * n, 0, b0);
        LaneTaps<4> tt[6], t0[6];
        float vt[6], v0[6];
        const double gt = full_vals(pl, bt, ch, lane_on, tt, vt);
        const double g0 = full_vals(pl, b0, ch, lane_on, t0, v0);
        const double dgd = gt - g0;                                        // g_t - g_0 of this lane's channel (0 in lanes >= 48)
        const float dg = (float)dgd;
        double yd = 0.0;                                                   // lane j < 32: (W dg)_j, in double: the value path
#pragma unroll 8
        for (int c = 0; c < 48; ++c) yd += (double)Wl[jrow * PW_WSTRIDE + c] * lane_bcast(dgd, c);
        if (lane >= 32) yd = 0.0;
        lsum += wave_sum(yd * yd);
        const float y = (float)yd;
        float gl = 0.f;                                                    // lane c < 48: (W^T y)_c
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float yj = lane_bcast(y, j);
            gl += Wl[j * PW_WSTRIDE + ch] * yj;
            if (want_w) accW[j] += yj * dg;
        }
        gl *= a.s_a;
        char_scatter(gp, tt, vt, gl);
        char_scatter(gp, t0, v0, -gl);
    }
    if (lane == 0 && lsum != 0.0) atomicAdd(a.acc + 1, lsum);
    if (want_w) flush_dw(accW, red, ch, lane_on, f.app_dim, a.s_a, a.g.basis);
}

__global__ void k_char_times(int64_t N, float t, float* tt, float* tb) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < N) { tt[i] = t; tb[i] = 0.f; }
}
// t_k == 0: both lookups are the same lookup - exact zeros, x0 = x, no gradient is touched
__global__ void k_char_zero(int64_t N, const float* x, float* x0_out, float* loss) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < 2) loss[i] = 0.f;
    if (x0_out && i < 3 * N) x0_out[i] = x[i];
}
__global__ void k_char_finish(const double* acc, double inv_d, double inv_a, float* loss) {
    if (threadIdx.x < 2) loss[threadIdx.x] = (float)(acc[threadIdx.x] * (threadIdx.x ? inv_a : inv_d));
}

// the reference's snap (tensorf_keyframe.py:554-561): t > 0 -> the nearest keyframe time, otherwise the FIRST keyframe interval ts
static int char_row(const nvfi_field_desc& f, float t, float* tk) {
    if (t > 0.f) {
        const float ts = time_scale(f), hi = (float)(f.K - 1);
        float q = t / ts;
        if (q < 0.f) q = 0.f;
        if (q > hi) q = hi;
        q = rintf(q);
        *tk = q * ts;
        return (int)q;
    }
    *tk = f.tmax / (float)(f.K - 1);
    return 1;
}
struct CharPlan { double* acc; float* tt; float* tb; float* x0; char* vel; int64_t vel_bytes; int64_t total; };
static void plan_char(const nvfi_field_desc* f, int64_t N, void* ws, CharPlan* P) {
    Bump B{(char*)ws, 0, 0};
    P->acc = B.take<double>(2);
    P->tt = B.take<float>(N);
    P->tb = B.take<float>(N);
    P->x0 = B.take<float>(3 * N);
    nvfi_vel_workspace_bytes(f, N, &P->vel_bytes);
    P->vel = B.take<char>(P->vel_bytes);
    P->total = align_up(B.off, 256);
}
extern "C" int nvfi_char_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes) {
    CharPlan P; plan_char(f, N > 0 ? N : 0, nullptr, &P);
    *bytes = P.total;
    return 0;
}
extern "C" int nvfi_char_loss(const nvfi_field_desc* f, int64_t N, const float* points, float t, float weight, float* loss,
                              float* points0_out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0) return nvfi_fail(2, "nvfi_char_loss needs at least one point");
    if (N >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "N too large for one call; chunk the points");
    if (!f->use_vel) return nvfi_fail(2, "the characteristic loss needs the velocity field (use_vel = 0)");
    if (f->K < 2 || !(f->tmax > 0.f)) return nvfi_fail(2, "the characteristic loss needs at least two keyframes and tmax > 0");
    if (f->Cd != 24 || f->Ca != 48 || f->app_dim < 1 || f->app_dim > 32)
        return nvfi_fail(2, "characteristic loss: 24 density / 48 appearance components and app_dim <= 32 (got %d / %d / %d)", f->Cd, f->Ca, f->app_dim);
    float tk;
    const int row = char_row(*f, t, &tk);
    if (row == 0) {
        const int64_t n = 3 * N > 2 ? 3 * N : 2;
        hipLaunchKernelGGL(k_char_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, N, points, points0_out, loss);
        LAUNCHCK();
        return 0;
    }
    CharPlan P; plan_char(f, N, workspace, &P);
    if (P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)P.total);
    float* x0 = points0_out ? points0_out : P.x0;
    hipLaunchKernelGGL(k_char_times, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, tk, P.tt, P.tb);
    // the warp IS nvfi_integrate_pos: same launch path (x6 by default), same bits as the stand-alone call
    if (const int rc = nvfi_integrate_pos(f, N, points, P.tt, P.tb, x0, P.vel, P.vel_bytes, stream)) return rc;
    if (launch_zero(P.acc, 2 * sizeof(double), st)) return 1;
    CharArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.N = N; a.x = points; a.x0 = x0; a.row = row; a.acc = P.acc;
    if (grads) {
        for (int i = 0; i < 3; ++i) { a.g.dps[i] = grads->dps[i]; a.g.dpt[i] = grads->dpt[i]; a.g.aps[i] = grads->aps[i]; a.g.apt[i] = grads->apt[i]; }
        a.g.basis = grads->basis;
    }
    a.s_d = (float)((double)weight * 2.0 / (double)N);
    a.s_a = (float)((double)weight * 2.0 / ((double)N * (double)f->app_dim));
    const unsigned nb = point_grid(N, 2);                                  // (k_char_app flushes dW per workgroup)
    hipLaunchKernelGGL(k_char_density, dim3(nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_char_app, dim3(nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_char_finish, dim3(1), dim3(64), 0, st, P.acc, 1.0 / (double)N, 1.0 / ((double)N * (double)f->app_dim), loss);
    LAUNCHCK();
    return 0;
}
