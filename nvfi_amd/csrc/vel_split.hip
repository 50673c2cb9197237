// vel_split.hip - fp32 RK2 back-advection (reference models/tensorf_keyframe.py:575-611 around the gated VelBasis of
// models/velocity_field.py:21-98) with the network's FEATURES split over the four waves of a workgroup:
//   k_rk2_split       per-point times, one 32-point tile per workgroup: the fp32 PDE prefilter and the fp32 re-evaluation list behind the
//                     16-bit pre-passes (NVFI_PDE_PREFILTER=fp32 / the band list of pre16.hip);
//   k_rk2_split_uni   the render warp (uniform step schedule, optional training stash), two tiles per workgroup (NVFI_RK2_X6=0);
//   k_rk2_split_bwd   its adjoint, two tiles per workgroup (NVFI_RK2_FUSE=0); <true>: with the gradient at the starting position (nvfi_advect_grad).
//
// k_rk2_fwd (vel.hip) gives every wave its own tile: best throughput per staged weight byte, but a tile's latency is the whole
// network on one SIMD (~100 k cycles per evaluation), which is what a SHORT list of points pays however few they are.  Here wave w owns
// output rows [32w, 32w + 32) of every hidden layer (one MFMA tile, the x4 weight fragments of pde_jet.hip read straight from L2 into
// registers one layer ahead) and the four 32-row slices meet in a 16 KB LDS exchange buffer between layers.  A tile's latency drops ~3.5x.
//
// Every hidden-layer accumulator sees the same operands in the same K order as in engine.h's layer_tiles, and every wave carries the same
// replicated RK2 state.  The render warp contracts the 128 -> 6 output layer on the matrix pipe too (one wave per tile, rotating with the
// workgroup index, broadcast through LDS): its results are k_rk2_fwd<true>'s bit for bit.  k_rk2_split forms it on the vector pipe.
#include <stdlib.h>
#include "common.h"
#include "vel.h"
#include "pde.h"

#define SPLIT_XCH_F4 (16 * 64)              // [s/4][lane] float4: one layer's 128 features x 32 points
#define SPLIT_NT 2                          // tiles per workgroup of the render warp and its adjoint: every 16-byte weight load feeds two tiles

template <int NS4>
__device__ __forceinline__ void split_load(const float4* __restrict__ a4, int lane, float4* wq) {
#pragma unroll
    for (int g = 0; g < NS4; ++g) wq[g] = a4[g * 64 + lane];
}
// layer 0: the 16 encoder slots of NT tiles (registers) against the four weight groups in wq
template <int NT>
__device__ __forceinline__ void split_mfma0(const float4* wq, const float (*x)[16], f32x16* acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float av[4] = {wq[g].x, wq[g].y, wq[g].z, wq[g].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = MFMA32(av[k], x[t][4 * g + k], acc[t]);
    }
}

// a hidden layer: the B operands streamed from the exchange buffer (one 16-byte LDS read per tile and 4 K-steps): no register copy of
// the layer input, and every 16-byte weight load feeds 4 NT MFMAs
template <int NT>
__device__ __forceinline__ void split_mfma_lds(const float4* wq, const float4* xl, int tile0, f32x16* acc) {
    float4 b[NT], bn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b[t] = xl[((tile0 + t) * 16) * 64];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if (g + 1 < 16) {
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[t] = xl[((tile0 + t) * 16 + g + 1) * 64];
        }
        const float av[4] = {wq[g].x, wq[g].y, wq[g].z, wq[g].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float bv = k == 0 ? b[t].x : (k == 1 ? b[t].y : (k == 2 ? b[t].z : b[t].w));
                acc[t] = MFMA32(av[k], bv, acc[t]);
            }
#pragma unroll
        for (int t = 0; t < NT; ++t) b[t] = bn[t];
    }
}

// one gated-velocity network evaluation of the workgroup's SPLIT_NT tiles, every layer on the matrix pipe; all four waves return the same out4
// (lane h=0: w0..w3, h=1: w4, w5) per tile
// STASH (training render): pre-activations z (5 layers x 64 rows, wave w = rows 16w..16w+15 of each layer) and the encoder slots go to
// the per-(evaluation, tile) stash in exactly the layout of velnet_forward (engine.h), so the adjoint and k_wgrad_ring8 read it unchanged
template <bool STASH>
__device__ __forceinline__ void velnet_split(const float4* const* f4, float4* xch, float* bc, int w, int owner, int lane, int h,
                                             const float4* q, float4* wq, const float* lb, float (&out4)[SPLIT_NT][4],
                                             float* const* zst, float* const* x0st) {
    constexpr int NT = SPLIT_NT;
    f32x16 acc[NT];
    const float4* xl = xch + lane;
    {
        float in0[NT][16];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            vel_encode_slots(q[t], h, in0[t]);
            if (STASH && w == t) stash_store<16>(x0st[t], lane, in0[t]);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = lb[32 * w + (r & 3) + 8 * (r >> 2) + 4 * h];
        }
        split_mfma0<NT>(wq, in0, acc);                   // wq holds layer 0 (loaded by the caller / the previous evaluation)
    }
    const int mine = (w - owner) & 3;                    // the tile whose 128 -> 6 output layer this wave contracts (if < NT)
#pragma unroll 1
    for (int l = 0; l < 5; ++l) {
        // the next layer's weights start their trip from L2 now; they land behind the epilogue and the exchange
        if (l < 4) split_load<16>(f4[l + 1] + (size_t)w * 16 * 64, lane, wq);
        else if (mine < NT) split_load<16>(f4[5], lane, wq);
        if (STASH) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) STASH_ST(zst[t][(size_t)(l * 64 + 16 * w + r) * REGF + lane], acc[t][r]);
        }
        __syncthreads();                                 // the previous layer's readers of the exchange buffer are done
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                xch[(t * 16 + 4 * w + k) * 64 + lane] = make_float4(act_f<1>(acc[t][4 * k]), act_f<1>(acc[t][4 * k + 1]), act_f<1>(acc[t][4 * k + 2]),
                                                                    act_f<1>(acc[t][4 * k + 3]));
        __syncthreads();
        if (l < 4) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = lb[128 * (l + 1) + 32 * w + (r & 3) + 8 * (r >> 2) + 4 * h];
            split_mfma_lds<NT>(wq, xl, 0, acc);
        }
    }
    // 128 -> 6 output layer: tile t is contracted by wave (owner + t) & 3 alone (one accumulator, K in layer_tiles' order)
    if (mine < NT) {
        f32x16 ao[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) ao[0][r] = lb[128 * 5 + (r & 3) + 8 * (r >> 2) + 4 * h];
        split_mfma_lds<1>(wq, xl, mine, ao);
#pragma unroll
        for (int r = 0; r < 4; ++r) bc[(mine * 4 + r) * 64 + lane] = ao[0][r];
    }
    // layer 0 of the NEXT evaluation (the caller stops using wq before that)
    split_load<4>(f4[0] + (size_t)w * 4 * 64, lane, wq);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out4[t][r] = bc[(t * 4 + r) * 64 + lane];
}

// ---------------------------------------------------------------- one tile, the 128 -> 6 OUTPUT layer on the vector pipe
// On the matrix pipe the output layer is 64 MFMAs of a 32-row tile that holds 6 useful rows, issued by one wave per tile while the
// other waves of the workgroup wait at the barrier behind it: 10 % of an evaluation's critical path for 0.5 % of its arithmetic.
// Here every lane multiplies the 16 activations of the last hidden layer it already holds in registers (its point i, features
// 32 w + (r & 3) + 8 (r >> 2) + 4 h) with the matching 16 x 6 output weights (the vel_stage_w5 image, 4 KB of LDS), the two halves meet by
// one cross-lane add, the four waves' partial sums by one trip through LDS (part: [wave][2][32 points] float4, added in wave order by every
// wave: replicated state stays bit-identical across the workgroup), and the last hidden layer's activations never go to the exchange buffer.
// fp32 FMAs in a fixed order instead of the MFMA's products and sums: the same arithmetic, another rounding (1e-7 relative).
// (velnet_x6 of vel_x6.hip ends with the same statements for its NT tiles; that unit's instructions must not move, so they stay there.)
__device__ __forceinline__ void velnet_split_vout(const float4* const* f4, float4* xch, float4* part, const float4* w5l, int w, int lane, int h,
                                                  const float4& q, float4* wq, const float* lb, float (&out6)[6]) {
    f32x16 acc;
    const float4* xl = xch + lane;
    {
        float in0[16];
        vel_encode_slots(q, h, in0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = lb[32 * w + (r & 3) + 8 * (r >> 2) + 4 * h];
        split_mfma0<1>(wq, &in0, &acc);                  // wq holds layer 0 (loaded by the caller / the previous evaluation)
    }
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        split_load<16>(f4[l + 1] + (size_t)w * 16 * 64, lane, wq);
        __syncthreads();                                 // the previous layer's readers of the exchange buffer are done
#pragma unroll
        for (int k = 0; k < 4; ++k)
            xch[(4 * w + k) * 64 + lane] = make_float4(act_f<1>(acc[4 * k]), act_f<1>(acc[4 * k + 1]), act_f<1>(acc[4 * k + 2]), act_f<1>(acc[4 * k + 3]));
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = lb[128 * (l + 1) + 32 * w + (r & 3) + 8 * (r >> 2) + 4 * h];
        split_mfma_lds<1>(wq, xl, 0, &acc);
    }
    // layer 0 of the NEXT evaluation (the caller stops using wq before that)
    split_load<4>(f4[0] + (size_t)w * 4 * 64, lane, wq);
    float p[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) p[o] = 0.f;
    const float4* wl = w5l + (w * 2 + h) * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if ((r & 1) == 0) __builtin_amdgcn_sched_barrier(0);     // weight reads in groups of two rows (all 32 at once cost 128 registers)
        const float4 wa = wl[2 * r], wb = wl[2 * r + 1];
        const float av = act_f<1>(acc[r]);
        p[0] = __builtin_fmaf(av, wa.x, p[0]); p[1] = __builtin_fmaf(av, wa.y, p[1]); p[2] = __builtin_fmaf(av, wa.z, p[2]);
        p[3] = __builtin_fmaf(av, wa.w, p[3]); p[4] = __builtin_fmaf(av, wb.x, p[4]); p[5] = __builtin_fmaf(av, wb.y, p[5]);
    }
#pragma unroll
    for (int o = 0; o < 6; ++o) p[o] += __shfl_xor(p[o], 32);
    if (h == 0) {
        part[(w * 2 + 0) * 32 + lane] = make_float4(p[0], p[1], p[2], p[3]);
        part[(w * 2 + 1) * 32 + lane] = make_float4(p[4], p[5], 0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < 6; ++o) out6[o] = lb[128 * 5 + o];
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
        __builtin_amdgcn_sched_barrier(0);
        const float4 A = part[(ww * 2 + 0) * 32 + (lane & 31)], B = part[(ww * 2 + 1) * 32 + (lane & 31)];
        out6[0] += A.x; out6[1] += A.y; out6[2] += A.z; out6[3] += A.w; out6[4] += B.x; out6[5] += B.y;
    }
}

// exchange buffer + [wave][2][32 points] float4 partial output sums + six bias vectors + the vel_stage_w5 image
#define SPLIT_VOUT_LDS_BYTES (SPLIT_XCH_F4 * 16 + 4 * 2 * 32 * 16 + 6 * 128 * 4 + VEL_W5_FLOATS * 4)
// One tile per workgroup: alone it is 1.5 % slower than two (1.32 against 1.30 ms; every weight load feeds one tile), but its 126-register
// workgroups leave the render chains' kernels more room beside it - the three-stream step is 1 % faster (5.04 against 5.10 ms).
// Four workgroups per CU (three: prefilter 1.31 instead of 1.29 ms)
#define SPLIT_WG_PER_CU_1 4
__global__ __launch_bounds__(WG_THREADS, SPLIT_WG_PER_CU_1) void k_rk2_split(SplitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float4* xch = reinterpret_cast<float4*>(lds);
    float4* part = xch + SPLIT_XCH_F4;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int count = a.count ? *a.count : (int)a.n_direct;
    if ((int)blockIdx.x * TILE >= count) return;
    const int i = blockIdx.x * TILE + (lane & 31);
    const bool active = i < count;
    const int n = active ? (a.list ? a.list[i] : i) : 0;
    const float4 q0 = active ? a.xw[n] : zero4();
    float x = q0.x, y = q0.y, z = q0.z;
    const float zw = q0.w;
    const int ti = a.pt_by_list ? n : i;
    float tcur = active ? a.pt_t[ti] : 0.f;
    float off = active ? tcur - a.pt_base[ti] : 0.f;
    float4 wq[16];
    split_load<4>(a.f4[0] + (size_t)w * 4 * 64, lane, wq);
    // the six bias vectors live in LDS for the whole kernel (3 KB; rows beyond a layer's width read as the fragment's zero padding) ...
    float* lb = reinterpret_cast<float*>(part + 4 * 2 * 32);
    vel_stage_biases(lb, a.bv, 32);
    // ... and so do the output layer's weights
    float* w5f = lb + 6 * 128;
    vel_stage_w5(w5f, a.f.vW[5]);
    const float4* w5l = reinterpret_cast<const float4*>(w5f);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < a.max_steps; ++s) {
        const bool live = active && fabsf(off) > 0.f;
        const float dt = rk2_point_dt(off, a.dt_max);
        if (!__any(live)) break;                          // the same decision in all four waves (replicated state)
        const float hdt = 0.5f * dt;
        float o6[6], px, py, pz, nx, ny, nz;
        velnet_split_vout(a.f4, xch, part, w5l, w, lane, h, make_float4(x, y, z, tcur), wq, lb, o6);
        rk2_midpoint(a.f, o6, x, y, z, hdt, px, py, pz);
        velnet_split_vout(a.f4, xch, part, w5l, w, lane, h, make_float4(px, py, pz, tcur - hdt), wq, lb, o6);
        const bool rej = rk2_final(a.f, o6, x, y, z, px, py, pz, dt, nx, ny, nz) & 4;
        if (live && !rej) { x = nx; y = ny; z = nz; }
        if (live) { off = off - dt; tcur = tcur - dt; }
    }
    if (active && h == 0 && w == 0) a.xw[n] = make_float4(x, y, z, zw);
}

// ---------------------------------------------------------------- render warp: every sample takes the same (dt_s, t_s) sequence
// (k_rk2_fwd<true> of vel.hip on the feature-split layout, with the training stash and records: same numbers)
// The output layer stays on the matrix pipe here.  On the vector pipe as in k_rk2_split the kernel alone gains 5.5 % (0.475 -> 0.447 ms per
// step, 0.59 -> 0.63 of the fp32 MFMA peak), but the allocator then takes 228 / 204 registers instead of 179 / 150, the gather / scatter
// kernels of the other chains no longer fit beside its two waves per SIMD, and the three-stream step gains nothing (5.04 against 5.07 ms)
#define SPLIT_UNI_LDS_BYTES (SPLIT_NT * (SPLIT_XCH_F4 * 16 + 4 * 64 * 4) + 6 * 128 * 4)
// PT (nvfi_advect_grad_pt, advect_pt.hip): every sample reads its own (dt, start time) of step s from the schedule table ra.pt_t / ra.pt_base
// ([s][compact index], ra.cap apart); a sample whose dt is 0 there has finished: the step leaves it where it is and records flag 4
template <bool STASH, bool PT = false>
__global__ __launch_bounds__(WG_THREADS, 2) void k_rk2_split_uni(SplitUniArgs a) {
    constexpr int NT = SPLIT_NT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float4* xch = reinterpret_cast<float4*>(lds);
    float* bc = reinterpret_cast<float*>(xch + NT * SPLIT_XCH_F4);       // the 4 x 64 broadcast rows of every tile's output layer
    const Rk2Args& ra = a.r;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int owner = blockIdx.x & 3;
    const int count = *ra.count;
    // whole 128-sample groups, as k_rk2_fwd: the adjoint and weight-gradient kernels walk every tile of the last, ragged group
    if ((int)blockIdx.x * NT * TILE >= (count + WG_SAMPLES - 1) / WG_SAMPLES * WG_SAMPLES) return;
    bool active[NT]; int n[NT], idx[NT]; float x[NT], y[NT], z[NT], zw[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        idx[t] = (blockIdx.x * NT + t) * TILE + (lane & 31);
        active[t] = idx[t] < count;
        n[t] = active[t] ? ra.list[idx[t]] : 0;
        const float4 q0 = active[t] ? ra.xw[n[t]] : zero4();
        x[t] = q0.x; y[t] = q0.y; z[t] = q0.z; zw[t] = q0.w;
    }
    float4 wq[16];
    split_load<4>(a.f4[0] + (size_t)w * 4 * 64, lane, wq);
    float* lb = bc + NT * 4 * 64;
    vel_stage_biases(lb, a.bv, 32);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < ra.nsteps; ++s) {
        const float dt = PT ? 0.f : RK_DT(ra, s), tcur = PT ? 0.f : RK_TC(ra, s), hdt = 0.5f * dt;
        float dtp[NT], tcp[NT];
        if constexpr (PT) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const size_t o = (size_t)s * ra.cap + (active[t] ? idx[t] : 0);
                dtp[t] = active[t] ? ra.pt_t[o] : 0.f; tcp[t] = active[t] ? ra.pt_base[o] : 0.f;
            }
        }
        float* z1[NT]; float* z2[NT]; float* x1[NT]; float* x2[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const size_t tile = (size_t)blockIdx.x * NT + t;
            const size_t e1 = (size_t)(2 * s) * ra.cap_tiles + tile, e2 = (size_t)(2 * s + 1) * ra.cap_tiles + tile;
            z1[t] = STASH ? ra.zst + e1 * (VEL_Z_REGS * REGF) : nullptr; z2[t] = STASH ? ra.zst + e2 * (VEL_Z_REGS * REGF) : nullptr;
            x1[t] = STASH ? ra.x0st + e1 * (VEL_X0_REGS * REGF) : nullptr; x2[t] = STASH ? ra.x0st + e2 * (VEL_X0_REGS * REGF) : nullptr;
        }
        float o4[NT][4], px[NT], py[NT], pz[NT], w1[NT][6];
        int g1[NT];
        float4 q[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) q[t] = make_float4(x[t], y[t], z[t], PT ? tcp[t] : tcur);
        velnet_split<STASH>(a.f4, xch, bc, w, owner, lane, h, q, wq, lb, o4, z1, x1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            gather6(o4[t], h, w1[t]);
            g1[t] = rk2_midpoint(ra.f, w1[t], x[t], y[t], z[t], PT ? 0.5f * dtp[t] : hdt, px[t], py[t], pz[t]);
            q[t] = make_float4(px[t], py[t], pz[t], PT ? tcp[t] - 0.5f * dtp[t] : tcur - hdt);
        }
        velnet_split<STASH>(a.f4, xch, bc, w, owner, lane, h, q, wq, lb, o4, z2, x2);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float w2[6], nx, ny, nz;
            gather6(o4[t], h, w2);
            const int g2rej = rk2_final(ra.f, w2, x[t], y[t], z[t], px[t], py[t], pz[t], PT ? dtp[t] : dt, nx, ny, nz) | (PT && dtp[t] == 0.f ? 4 : 0);
            if (STASH && active[t] && h == 0 && w == (t & 3))
                rk2_record_store(ra.rec + (size_t)s * RK_NF * ra.cap + idx[t], ra.cap, x[t], y[t], z[t], px[t], py[t], pz[t], w1[t], w2, g1[t] | g2rej);
            if (active[t] && !(g2rej & 4)) { x[t] = nx; y[t] = ny; z[t] = nz; }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (active[t] && h == 0 && w == 0) ra.xw[n[t]] = make_float4(x[t], y[t], z[t], zw[t]);
}

int launch_rk2_split_uni(const SplitUniArgs& a, int64_t cap_samples, bool stash, hipStream_t st) {
    const int64_t tiles = (cap_samples + TILE - 1) / TILE;
    if (tiles <= 0) return 0;
    ProfScope ps(PK_RK2_FWD, st);
    const dim3 g((unsigned)((tiles + SPLIT_NT - 1) / SPLIT_NT)), b(WG_THREADS);
    if (stash) hipLaunchKernelGGL(k_rk2_split_uni<true>, g, b, SPLIT_UNI_LDS_BYTES, st, a);
    else hipLaunchKernelGGL(k_rk2_split_uni<false>, g, b, SPLIT_UNI_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}

// the per-point-times stash form (nvfi_advect_grad_pt)
int launch_rk2_split_uni_pt(const SplitUniArgs& a, int64_t cap_samples, hipStream_t st) {
    const int64_t tiles = (cap_samples + TILE - 1) / TILE;
    if (tiles <= 0) return 0;
    ProfScope ps(PK_RK2_FWD, st);
    const dim3 g((unsigned)((tiles + SPLIT_NT - 1) / SPLIT_NT)), b(WG_THREADS);
    hipLaunchKernelGGL((k_rk2_split_uni<true, true>), g, b, SPLIT_UNI_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}

// ---------------------------------------------------------------- RK2 adjoint of the render warp on the same layout
// (the adjoint of k_rk2_split_uni<true>: same recurrence, same stash rows, K in layer_tiles' order per accumulator.)
// Wave w owns rows [32w, 32w + 32) of every layer's INPUT gradient (one tile of the transposed weights, x4 fragments from L2), loads
// only its own 16 z rows and stores only its own 16 adjoint rows per layer and tile; the 128 -> 28 input layer of tile t is
// contracted by wave (owner + t) & 3 and its 16 slot gradients are broadcast through LDS.  40 KB of LDS: the kernel shares a CU with
// whatever the other streams run.
#define SPLIT_BWD_LDS_BYTES (SPLIT_NT * (SPLIT_XCH_F4 * 16 + 16 * 64 * 4))

__device__ __forceinline__ void velnet_split_bwd(const float4* const* t4, float4* xch, float* bc, int w, int owner, int lane,
                                                 const float (&gw4)[SPLIT_NT][4], const float* const* zst, float* const* gst, float4* wq,
                                                 float (&ge)[SPLIT_NT][16]) {
    constexpr int NT = SPLIT_NT;
    f32x16 acc[NT];
    float zp[NT][16];
    const float4* xl = xch + lane;
    const int mine = (w - owner) & 3;
    wq[0] = t4[5][(size_t)w * 64 + lane];                 // T5: 4 tiles x 1 group of 4 K-steps
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) zp[t][r] = STASH_LD(zst[t][(size_t)(4 * 64 + 16 * w + r) * REGF + lane]);
        if (w == t) {                                     // adjoint of the 6 outputs: B operand of the output layer's weight gradient
            float* gw_rows = gst[t] + (size_t)5 * 64 * REGF;
#pragma unroll
            for (int r = 0; r < 16; ++r) gw_rows[r * REGF + lane] = r < 4 ? gw4[t][r] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    }
    {
        const float av[4] = {wq[0].x, wq[0].y, wq[0].z, wq[0].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = MFMA32(av[k], gw4[t][k], acc[t]);
    }
#pragma unroll 1
    for (int l = 4; l >= 0; --l) {
        if (l >= 1) split_load<16>(t4[l] + (size_t)w * 16 * 64, lane, wq);
        else if (mine < NT) split_load<16>(t4[0], lane, wq);
        float g[NT][16];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                g[t][r] = acc[t][r] * act_d1<1>(zp[t][r]);
                STASH_ST(gst[t][(size_t)(l * 64 + 16 * w + r) * REGF + lane], g[t][r]);
            }
            if (l >= 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) zp[t][r] = STASH_LD(zst[t][(size_t)((l - 1) * 64 + 16 * w + r) * REGF + lane]);
            }
        }
        __syncthreads();                                  // the previous layer's readers of the exchange buffer are done
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                xch[(t * 16 + 4 * w + k) * 64 + lane] = make_float4(g[t][4 * k], g[t][4 * k + 1], g[t][4 * k + 2], g[t][4 * k + 3]);
        __syncthreads();
        if (l >= 1) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            split_mfma_lds<NT>(wq, xl, 0, acc);
        }
    }
    if (mine < NT) {
        f32x16 ao[1];
#pragma unroll
        for (int r = 0; r < 16; ++r) ao[0][r] = 0.f;
        split_mfma_lds<1>(wq, xl, mine, ao);
#pragma unroll
        for (int r = 0; r < 16; ++r) bc[(mine * 16 + r) * 64 + lane] = ao[0][r];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ge[t][r] = bc[(t * 16 + r) * 64 + lane];
}

// GX0 (nvfi_advect_grad): the gradient that is left in g3 after the last (= first forward) step goes to a.gx0 - the one output the render never
// needed, its samples being constants.  The render launches the plain instantiation
// PT (nvfi_advect_grad_pt): dt and the start time of step s are the sample's own, from the table the PT forward read (ra.pt_t / ra.pt_base); a
// finished sample's step carries record flag 4 and is the identity, like a rejected one
template <bool GX0, bool PT = false>
__global__ __launch_bounds__(WG_THREADS, 2) void k_rk2_split_bwd(SplitBwdArgs a) {
    constexpr int NT = SPLIT_NT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float4* xch = reinterpret_cast<float4*>(lds);
    float* bc = lds + NT * SPLIT_XCH_F4 * 4;
    const Rk2Args& ra = a.r;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int owner = blockIdx.x & 3;
    const int count = *ra.count;
    if ((int)blockIdx.x * NT * TILE >= (count + WG_SAMPLES - 1) / WG_SAMPLES * WG_SAMPLES) return;
    bool active[NT]; int idx[NT]; float g3[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        idx[t] = (blockIdx.x * NT + t) * TILE + (lane & 31);
        active[t] = idx[t] < count;
        const float4 gin = active[t] ? ra.gxk[ra.list[idx[t]]] : zero4();   // upstream gradient of the warped position
        g3[t][0] = gin.x; g3[t][1] = gin.y; g3[t][2] = gin.z;
    }
    float4 wq[16];
#pragma unroll 1
    for (int s = ra.nsteps - 1; s >= 0; --s) {
        const float dt = PT ? 0.f : RK_DT(ra, s), tcur = PT ? 0.f : RK_TC(ra, s);
        float dtp[NT], tcp[NT];
        if constexpr (PT) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const size_t o = (size_t)s * ra.cap + (active[t] ? idx[t] : 0);
                dtp[t] = active[t] ? ra.pt_t[o] : 0.f; tcp[t] = active[t] ? ra.pt_base[o] : 0.f;
            }
        }
        float gacc[NT][3], gup[NT][3];
        bool g1[NT], g2[NT], rej[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float* rc = ra.rec + (size_t)s * RK_NF * ra.cap + (active[t] ? idx[t] : 0);
            const int flags = active[t] ? __float_as_int(rc[18 * ra.cap]) : 7;
            g1[t] = flags & 1; g2[t] = flags & 2; rej[t] = flags & 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) { gacc[t][c] = 0.f; gup[t][c] = g3[t][c]; }
        }
#pragma unroll 1
        for (int e = 1; e >= 0; --e) {
            const int po = e ? 3 : 0, wo = e ? 12 : 6;
            const float coef = e ? -dt : -0.5f * dt;
            const float te = e ? tcur - 0.5f * dt : tcur;
            float r4[NT][4], gloc[NT][3], ge[NT][16];
            const float* zs[NT]; float* gs[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float* rc = ra.rec + (size_t)s * RK_NF * ra.cap + (active[t] ? idx[t] : 0);
                const bool gate = e ? g2[t] : g1[t];
                const size_t es = (size_t)(2 * s + e) * ra.cap_tiles + (size_t)blockIdx.x * NT + t;
                zs[t] = ra.zst + es * (VEL_Z_REGS * REGF); gs[t] = ra.gst + es * (VEL_G_REGS * REGF);
                float p[3], wv[6], gv[3], gw[6];
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = active[t] ? rc[(po + c) * ra.cap] : 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k) wv[k] = active[t] ? rc[(wo + k) * ra.cap] : 0.f;
                const bool on = active[t] && !rej[t] && !gate;
#pragma unroll
                for (int c = 0; c < 3; ++c) gv[c] = on ? (PT ? (e ? -dtp[t] : -0.5f * dtp[t]) : coef) * gup[t][c] : 0.f;
                gw[0] = gv[0]; gw[1] = gv[1]; gw[2] = gv[2];
                gw[3] = p[2] * gv[1] - p[1] * gv[2];
                gw[4] = -p[2] * gv[0] + p[0] * gv[2];
                gw[5] = p[1] * gv[0] - p[0] * gv[1];
                gloc[t][0] = -wv[5] * gv[1] + wv[4] * gv[2];
                gloc[t][1] = wv[5] * gv[0] - wv[3] * gv[2];
                gloc[t][2] = -wv[4] * gv[0] + wv[3] * gv[1];
                scatter6(gw, h, r4[t]);
            }
            velnet_split_bwd(a.t4, xch, bc, w, owner, lane, r4, zs, gs, wq, ge);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float* rc = ra.rec + (size_t)s * RK_NF * ra.cap + (active[t] ? idx[t] : 0);
                float p[3], x0[16];
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = active[t] ? rc[(po + c) * ra.cap] : 0.f;
                vel_encode_slots(make_float4(p[0], p[1], p[2], PT ? (e ? tcp[t] - 0.5f * dtp[t] : tcp[t]) : te), h, x0);
                const float4 gq = vel_encode_bwd(ge[t], x0, h);
                gloc[t][0] += gq.x; gloc[t][1] += gq.y; gloc[t][2] += gq.z;
#pragma unroll
                for (int c = 0; c < 3; ++c) { gacc[t][c] += gloc[t][c]; gup[t][c] = gloc[t][c]; }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (active[t] && !rej[t]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) g3[t][c] = g3[t][c] + gacc[t][c] + 0.f;
            }
    }
    if (GX0) {      // replicated state: every wave and both lane halves hold the same g3; one lane per point stores
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (active[t] && h == 0 && w == (t & 3)) {
                float* o = a.gx0 + 3 * (size_t)ra.list[idx[t]];
                o[0] = g3[t][0]; o[1] = g3[t][1]; o[2] = g3[t][2];
            }
    }
}

int launch_rk2_split_bwd(const SplitBwdArgs& a, int64_t cap_samples, hipStream_t st, bool want_gx0) {
    const int64_t tiles = (cap_samples + TILE - 1) / TILE;
    if (tiles <= 0) return 0;
    ProfScope ps(PK_RK2_BWD, st);
    const dim3 g((unsigned)((tiles + SPLIT_NT - 1) / SPLIT_NT)), b(WG_THREADS);
    if (want_gx0 && a.gx0) hipLaunchKernelGGL(k_rk2_split_bwd<true>, g, b, SPLIT_BWD_LDS_BYTES, st, a);
    else hipLaunchKernelGGL(k_rk2_split_bwd<false>, g, b, SPLIT_BWD_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}

// the per-point-times adjoint (nvfi_advect_grad_pt); a.gx0 may be NULL
int launch_rk2_split_bwd_pt(const SplitBwdArgs& a, int64_t cap_samples, hipStream_t st) {
    const int64_t tiles = (cap_samples + TILE - 1) / TILE;
    if (tiles <= 0) return 0;
    ProfScope ps(PK_RK2_BWD, st);
    const dim3 g((unsigned)((tiles + SPLIT_NT - 1) / SPLIT_NT)), b(WG_THREADS);
    if (a.gx0) hipLaunchKernelGGL((k_rk2_split_bwd<true, true>), g, b, SPLIT_BWD_LDS_BYTES, st, a);
    else hipLaunchKernelGGL((k_rk2_split_bwd<false, true>), g, b, SPLIT_BWD_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}

int launch_rk2_split(const SplitArgs& a, int64_t cap_points, hipStream_t st) {
    const int64_t tiles = (cap_points + TILE - 1) / TILE;
    if (tiles <= 0) return 0;
    ProfScope ps(PK_PDE_PREFILTER, st);
    hipLaunchKernelGGL(k_rk2_split, dim3((unsigned)tiles), dim3(WG_THREADS), SPLIT_VOUT_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}
