// pointwave.h - one wave per point, lanes are channels: the family of charloss.hip and lookup.hip (scatter_atomic.hip, the render backward's
// scatter, has the same layout over the render's sample list and keeps its own code: DET fixed point goes through its adds).
// A wave walks the points with a grid stride; per-point quantities (coordinates, the six tap sets Bl b[6] of a plane family - space 0..2,
// time 3..5) are wave-uniform, a tap is one contiguous texel vector:
//   density (24 channels)  lane = 2 * channel + x-tap: one load / atomic instruction covers two neighbouring texels (192 B); lanes >= 48 idle
//   appearance (48)        lane = channel: one texel per instruction (192 B); lanes >= 48 idle
// basis_mat (app_dim x 48) sits in LDS with an odd row stride, rows >= app_dim zero; dW is kept in registers per wave (lane = column, one
// register per row), reduced per workgroup in LDS, and only then added to global memory.
// What is NOT here, because the two units differ in it: how a point's Bl sets are formed (lookup.hip: common.h's fp32 plane_setups with
// fully masked planes zeroed; charloss.hip: coordinates in double on an integer time row), how the taps are loaded (lookup.hip: unconditional
// loads at offsets clamped to 0 under the mask, then a select; charloss.hip: loads under the mask) and every value's arithmetic.
#pragma once
#include "common.h"

__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }      // a wave-uniform load, held in an SGPR
__device__ __forceinline__ float lane_bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double lane_bcast(double v, int l) {
    const long long q = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)q, l), hi = __builtin_amdgcn_readlane((int)(q >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// the wave-walk prologue: `for (int64_t n = w.wave0; n < N; n += w.wtot)` visits every point once
struct PointWalk {
    int lane; int64_t wave0, wtot;
    __device__ __forceinline__ PointWalk() {
        const int nwv = blockDim.x >> 6;
        lane = threadIdx.x & 63;
        wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * nwv + (threadIdx.x >> 6));
        wtot = (int64_t)gridDim.x * nwv;
    }
};
// the host's grid rule for 256-thread workgroups: at least four points per wave, at most `per_cu` workgroups per CU (a kernel that flushes dW
// per workgroup takes a small cap, so that the flush stays a small share)
static inline unsigned point_grid(int64_t N, int per_cu) {
    const int64_t want = (N + 15) / 16, cap = (int64_t)per_cu * device_cu_count();
    return (unsigned)(want < cap ? want : cap);
}
// the six planes of a family, or their gradient buffers: space 0..2, time 3..5
template <class P> __device__ __forceinline__ void family_planes(P const* space, P const* time, P* out) {
#pragma unroll
    for (int p = 0; p < 3; ++p) { out[p] = space[p]; out[3 + p] = time[p]; }
}

// ---- the two tap layouts: this lane's taps of one plane as element offset, mask (lane_on and in range) and bilinear weight.  The offsets are
// NOT clamped: a load at o[k] is valid under m[k] only
template <int NT> struct LaneTaps { size_t o[NT]; bool m[NT]; float w[NT]; };
// density: the lane's x-tap (dx0) in the two rows; wx is the x weight of that tap
__device__ __forceinline__ void density_taps(const Bl& b, int ch, int dx0, bool lane_on, LaneTaps<2>& t, float& wx) {
    t.m[0] = lane_on && (dx0 ? b.m1 : b.m0); t.m[1] = lane_on && (dx0 ? b.m3 : b.m2);
    wx = dx0 ? b.w : b.e;
    t.o[0] = (size_t)(b.base + dx0) * 24 + ch; t.o[1] = t.o[0] + (size_t)b.W * 24;
    t.w[0] = wx * b.s; t.w[1] = wx * b.n;
}
// appearance: all four taps
__device__ __forceinline__ void app_taps(const Bl& b, int ch, bool lane_on, LaneTaps<4>& t) {
    t.m[0] = lane_on && b.m0; t.m[1] = lane_on && b.m1; t.m[2] = lane_on && b.m2; t.m[3] = lane_on && b.m3;
    t.o[0] = (size_t)b.base * 48 + ch; t.o[1] = t.o[0] + 48; t.o[2] = t.o[0] + (size_t)b.W * 48; t.o[3] = t.o[2] + 48;
    t.w[0] = b.e * b.s; t.w[1] = b.w * b.s; t.w[2] = b.e * b.n; t.w[3] = b.w * b.n;
}
// g x weight into the lane's texels of a gradient plane (float atomics in arrival order: not repeatable)
template <int NT> __device__ __forceinline__ void scatter_taps(float* gp, const LaneTaps<NT>& t, float g) {
#pragma unroll
    for (int k = 0; k < NT; ++k)
        if (t.m[k]) atomicAdd(gp + t.o[k], t.w[k] * g);
}

// the product of a channel's six bilinear values, and upstream x the product of the OTHER five for every plane
__device__ __forceinline__ float prod6(const float* v) { return ((v[0] * v[1]) * v[2]) * ((v[3] * v[4]) * v[5]); }
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

// ---- basis_mat in LDS
#define PW_WSTRIDE 49      // LDS row stride of basis_mat: odd, so lanes that read a column (row = lane) hit 32 different banks
// Wl[32 * PW_WSTRIDE] = basis_mat, rows >= app_dim zero; red[32 * 48] (the workgroup's dW, or NULL) = 0.  Every thread of the workgroup.
__device__ __forceinline__ void stage_basis(const nvfi_field_desc& f, float* Wl, float* red) {
    for (int k = threadIdx.x; k < 32 * 48; k += blockDim.x) {
        const int j = k / 48, c = k - 48 * j;
        Wl[j * PW_WSTRIDE + c] = j < f.app_dim ? f.basis[k] : 0.f;
        if (red) red[k] = 0.f;
    }
    __syncthreads();
}
// the dW flush: accW (this wave's rows of column ch) -> red -> scale x red added to g_basis.  Every thread of the workgroup, once.
__device__ __forceinline__ void flush_dw(const float* accW, float* red, int ch, bool lane_on, int app_dim, float scale, float* g_basis) {
    if (lane_on) {
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (accW[j] != 0.f) atomicAdd(&red[j * 48 + ch], accW[j]);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < app_dim * 48; k += blockDim.x)
        if (red[k] != 0.f) atomicAdd(g_basis + k, scale * red[k]);
}
