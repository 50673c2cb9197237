// pde_jet.h - the pieces the three jet kernels share (k_pde_jet_fwd / k_pde_jet_bwd of pde_jet.hip, k_pde_jet6_fwd of pde_jet6.hip): the encoder
// tangents, the fp32 MFMA loop over x4 fragments, the 128 -> 6 output stage, and the acceleration net's trailing workgroups.  Each unit keeps
// its own build flags (pde_jet6.hip: no SLP vectorisation); everything here is inlined into the kernel that calls it.
#pragma once
#include "common.h"
#include "pde.h"

#define JET_NC 5                                 // columns of a tile: value, d/dx, d/dy, d/dz, d/dt

// acc[c] += sum over NS4 groups of 4 K-steps:  A = this wave's x4 fragment (one 16-byte load per group, next group in flight),
// B = x[c][s_base + ...] for the five columns
template <int NS4, int XS>
__device__ __forceinline__ void jet_mfma(const float4* __restrict__ a4, int lane, const float (&x)[JET_NC][XS], int s_base, f32x16* acc) {
    float4 cur = a4[lane];
#pragma unroll
    for (int g = 0; g < NS4; ++g) {
        float4 nxt = cur;
        if (g + 1 < NS4) nxt = a4[(g + 1) * 64 + lane];
        const float av[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < JET_NC; ++c) acc[c] = MFMA32(av[k], x[c][s_base + 4 * g + k], acc[c]);
        cur = nxt;
    }
}

// tangent of the PositionEncoder slots wrt q_j
__device__ __forceinline__ void jet_encode_tangent(const float* x0, int h, int j, float* xd) {
#pragma unroll
    for (int s = 0; s < 16; ++s) xd[s] = 0.f;
    if (j == 0 && h == 0) xd[0] = 1.f;
    if (j == 1 && h == 1) xd[0] = 1.f;
    if (j == 2 && h == 0) xd[1] = 1.f;
    if (j == 3 && h == 1) xd[1] = 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float mine = x0[2 + 4 * k + c];
            const float other = __shfl_xor(mine, 32);
            const float fr = (float)(1 << k);
            if (c == j) xd[2 + 4 * k + c] = h ? -fr * other : fr * other;
        }
}

// output layer 128 -> 6 on the fp32 MFMA, split along K: this wave contracts its own 32 rows (x: the five columns' 16 activations), the partial
// sums meet in LDS and wave 0 stores the six outputs of every column to wout.  Called by all four waves of a jet tile; i: the lane's point
__device__ __forceinline__ void jet_output_stage(const PdeJetArgs& a, float* lds, const float (&x)[JET_NC][16], int w, int lane, int h, int i) {
    f32x16 acc[JET_NC];
#pragma unroll
    for (int c = 0; c < JET_NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    jet_mfma<4, 16>(a.f4[5] + (size_t)(4 * w) * 64, lane, x, 0, acc);
    __syncthreads();      // the exchange buffer's last readers are done
    float* red = lds;     // [wave][column][4 regs][64 lanes]
#pragma unroll
    for (int c = 0; c < JET_NC; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((w * JET_NC + c) * 4 + r) * 64 + lane] = acc[c][r];
    __syncthreads();
    if (w == 0 && h == 0 && i < a.cap) {
#pragma unroll
        for (int c = 0; c < JET_NC; ++c) {
            float o6[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                // output k lives in register k&3 of half k>>2 (D layout rows 0..3 | 4..7): lanes l (h=0) and l+32 (h=1)
                const int ln = lane + 32 * (k >> 2), r = k & 3;
                float s = c == 0 ? a.bv[5][k] : 0.f;
                s = s + red[((0 * JET_NC + c) * 4 + r) * 64 + ln];
                s = s + red[((1 * JET_NC + c) * 4 + r) * 64 + ln];
                s = s + red[((2 * JET_NC + c) * 4 + r) * 64 + ln];
                s = s + red[((3 * JET_NC + c) * 4 + r) * 64 + ln];
                o6[k] = s;
            }
            float* o = a.wout + (size_t)(c == 0 ? 0 : 6 * c) * a.cap + i;
#pragma unroll
            for (int k = 0; k < 6; ++k) o[(size_t)k * a.cap] = o6[k];
        }
    }
}

// Trailing workgroups of the jet launches (blockIdx.x >= jet_tiles): the ReLU acceleration net, whose Jacobian is not taken, for 4 tiles per
// workgroup - riding in these launches, its one round of workgroups fills the tail of the jet tiles instead of a launch of its own.
// forward: value column -> pre-activation stash + wout rows 30..35
__device__ __forceinline__ void jet_anet_forward(const PdeJetArgs& a, float* lds, int count, int w, int lane, int h) {
    const int wg = blockIdx.x - a.jet_tiles;
    if (wg * WG_SAMPLES >= count) return;
    const int tile = wg * 4 + w;
    const int i = tile * TILE + (lane & 31);
    const float4 q = i < count ? a.qorig[a.klist[a.first + i]] : zero4();
    float* T = a.stash + (size_t)tile * PDE_TILE_ROWS * REGF;
    float o4[4], aw[6];
    velnet_forward<0, true>(a.Wa, lds, lds + LDS_W_FLOATS, lane, q, T + PDE_ZA * REGF, nullptr, o4);
    gather6(o4, h, aw);
    if (h == 0 && i < a.cap) {
        float* o = a.wout + (size_t)30 * a.cap + i;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[(size_t)k * a.cap] = aw[k];
    }
}
// adjoint: seed rows 30..35 -> the value adjoint of velnet_value_backward (pde.h)
__device__ __forceinline__ void jet_anet_backward(const PdeJetArgs& a, float* lds, int count, int w, int lane, int h) {
    const int wg = blockIdx.x - a.jet_tiles;
    if (wg * WG_SAMPLES >= count) return;
    const int tile = wg * 4 + w;
    const int i = tile * TILE + (lane & 31);
    float* T = a.stash + (size_t)tile * PDE_TILE_ROWS * REGF;
    float r4[4], s6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s6[k] = i < (int)a.cap ? a.seeds[(size_t)(30 + k) * a.cap + i] : 0.f;
    scatter6(s6, h, r4);
    velnet_value_backward<0>(a.Wa, lds, lds + LDS_W_FLOATS, lane, r4, T + PDE_ZA * REGF, T + PDE_GAA * REGF);
}
