// vel.h - argument blocks of the velocity kernels (vel.hip)
#pragma once
#include "common.h"

#define RK_NF 19                       // per (step, sample) record fields: x3 pmid3 w1[6] w2[6] flags
#define VEL_G_REGS (5 * 64 + 16)       // adjoint stash rows per (eval, tile): gz[5][64] + gw[16]

struct VelEvalArgs {
    nvfi_field_desc f;
    VelFrags Wv, Wa;
    int64_t N;
    const float* xt;   // (N,4)
    float* u6;         // (N,6)
    int gated;
    const int* count;  // optional device-side count of points (<= N, which then sizes the grid): workgroups beyond it exit at once
    int u_stride;      // gated only: floats per point in u6, of which the first three are written (0: 6); the ungated (N,6) output has no stride
};

struct Rk2Args {
    nvfi_field_desc f;
    VelFrags Wv;
    const int* count;      // device count of compact samples (NULL -> n_direct)
    int64_t n_direct;
    const int* list;       // compact -> dense index (NULL: identity)
    float4* xw;            // dense (x,y,z,zval), updated in place unless xout
    float* xout;           // optional (count,3) output instead of in-place
    // uniform mode (render): per-step dt and start time
    int nsteps;
    float dt[MAX_RK_STEPS];
    float tcur[MAX_RK_STEPS];
    const float* sched;    // optional device-side schedule record (common.h): dt / tcur are read from it instead
    // per-point mode
    const float* pt_t; const float* pt_base; float dt_max; int max_steps;
    int pt_by_list;        // pt_t / pt_base are indexed by the dense index list[i] instead of the compact index i
    // (the stash kernels with per-point times - k_rk2_x6_uni_pt, k_rk2_split_uni<., true>, k_rk2_split_bwd<., true> - read pt_t / pt_base as the
    // schedule table of advect_pt.hip instead: dt[s][i] / tcur[s][i], i the compact index, `cap` apart, nsteps steps)
    // stashes (training)
    float* zst; float* x0st; float* rec; float* gst;
    int64_t cap; int64_t cap_tiles;
    int z_x4;              // the z rows of layers 0..3 are x4 stash blocks (engine.h: stash_st16_x4): written by the x6 warp kernels, read by the fused adjoint only
    // backward
    const float4* gxk;     // (dense, per sample) upstream gradient wrt the warped position
};

#ifdef __HIPCC__
// ---------------------------------------------------------------- the fp32 steps of the RK2 warp kernels
// Who calls what:
//   rk2_point_dt                          vel.hip, vel_split.hip, vel_x6.hip, vel_x6w.hip, pre16.hip (every per-point kernel)
//   rk2_midpoint, rk2_final               k_rk2_split, k_rk2_split_uni (vel_split.hip)
//   rk2_record_store                      k_rk2_split_uni<true>
//   vel_stage_biases / vel_stage_w5       k_rk2_split, k_rk2_split_uni / k_rk2_split
// These are NOT the only copies.  The same statements are still written out, and have to be kept in step BY HAND with a change made here, in:
//   the two halves of a step (gate, half step, full step, gate_sur rejection): vel.hip k_rk2_fwd; vel_x6.hip k_rk2_x6, k_rk2_x6_uni, k_rk2_x6_uni_pt;
//       vel_x6w.hip k_rk2_x6w, k_rk2_x6w_uni; pre16.hip k_rk2_pre16, k_rk2_inf16
//   the record store (RK_NF fields, flags last): vel_x6.hip k_rk2_x6_uni, k_rk2_x6_uni_pt; vel_x6w.hip k_rk2_x6w_uni; pre16.hip k_rk2_inf16; its readers are
//       k_rk2_split_bwd (vel_split.hip) and vel_fuse.hip
//   the bias / output-weight staging: vel_x6.hip (both kernels), vel_x6w.hip (both kernels)
// Why: calling the helpers there changed the compiled instructions.  vel_x6.hip, vel_x6w.hip and pre16.hip lie behind the packed-fp32 fence
// (build.py: NO_PACKED_F32), where code must not move without a hardware test of its own; in vel.hip both k_rk2_fwd kernels moved by a few
// instructions, and nothing in the benchmark times them, so they were left as they are too.
// per-point mode: the step a point takes next, min(|off|, dt_max) with the sign of off (off = time left to the base keyframe)
__device__ __forceinline__ float rk2_point_dt(float off, float dt_max) {
    const float m = fminf(fabsf(off), dt_max);
    return off > 0.f ? m : (off < 0.f ? -m : 0.f);
}
// first half of a step: gated velocity at (x, y, z) from the net's six outputs w1, half step to the midpoint p.  Returns record flag 1: gated
__device__ __forceinline__ int rk2_midpoint(const nvfi_field_desc& f, const float* w1, float x, float y, float z, float hdt, float& px, float& py, float& pz) {
    float v1[3];
    vel_from_w(w1, x, y, z, v1);
    const bool g1 = gated_out(f, x, y, z);
    if (g1) { v1[0] = v1[1] = v1[2] = 0.f; }
    px = x - hdt * v1[0]; py = y - hdt * v1[1]; pz = z - hdt * v1[2];
    return g1 ? 1 : 0;
}
// second half: gated velocity at the midpoint from w2, full step from (x, y, z) to n.  Returns record flags 2: gated at the midpoint |
// 4: n lies in the rejection box of VelocityAABBSur and the caller keeps (x, y, z)
__device__ __forceinline__ int rk2_final(const nvfi_field_desc& f, const float* w2, float x, float y, float z, float px, float py, float pz, float dt,
                                         float& nx, float& ny, float& nz) {
    float v2[3];
    vel_from_w(w2, px, py, pz, v2);
    const bool g2 = gated_out(f, px, py, pz);
    if (g2) { v2[0] = v2[1] = v2[2] = 0.f; }
    nx = x - dt * v2[0]; ny = y - dt * v2[1]; nz = z - dt * v2[2];
    const bool rej = f.gate_sur && gated_out(f, nx, ny, nz);   // tensorf_keyframe.py:603-605
    return (g2 ? 2 : 0) | (rej ? 4 : 0);
}
// the training record of one (step, sample): RK_NF fields, cap apart; rc = rec + step * RK_NF * cap + sample
__device__ __forceinline__ void rk2_record_store(float* rc, int64_t cap, float x, float y, float z, float px, float py, float pz, const float* w1,
                                                 const float* w2, int flags) {
    rc[0 * cap] = x; rc[1 * cap] = y; rc[2 * cap] = z;
    rc[3 * cap] = px; rc[4 * cap] = py; rc[5 * cap] = pz;
#pragma unroll
    for (int k = 0; k < 6; ++k) { rc[(6 + k) * cap] = w1[k]; rc[(12 + k) * cap] = w2[k]; }
    rc[18 * cap] = __int_as_float(flags);
}
// workgroup-wide staging into LDS (WG_THREADS threads; the caller's barrier follows).  lb[6][128]: the six bias vectors b[l], the last one `last`
// wide (32 in a packed fragment, 6 raw), zero beyond a layer's width
__device__ __forceinline__ void vel_stage_biases(float* lb, const float* const* b, int last) {
    for (int k = threadIdx.x; k < 6 * 128; k += WG_THREADS) lb[k] = (k & 127) < (k < 640 ? 128 : last) ? b[k >> 7][k & 127] : 0.f;
}
// w5f[4][2][16][8]: the 128 -> 6 output layer's weights W5 (6 x 128, row-major) in the order the lanes hold the last hidden layer - wave (row
// tile) w, lane half h, accumulator register r = feature 32 w + (r & 3) + 8 (r >> 2) + 4 h - as 6 outputs + 2 zeros
#define VEL_W5_FLOATS (4 * 2 * 16 * 8)
__device__ __forceinline__ void vel_stage_w5(float* w5f, const float* W5) {
    for (int k = threadIdx.x; k < VEL_W5_FLOATS; k += WG_THREADS) {
        const int o = k & 7, r = (k >> 3) & 15, hh = (k >> 7) & 1, ww = k >> 8;
        w5f[k] = o < 6 ? W5[o * 128 + 32 * ww + (r & 3) + 8 * (r >> 2) + 4 * hh] : 0.f;
    }
}
#endif

int launch_vel_eval(const VelEvalArgs& a, hipStream_t st);
// host callers: warp.hip (warp_points: the per-point form) and nvfi_compute_alpha's fixed-schedule branch (abi.hip: the only uniform caller)
int launch_rk2_fwd(const Rk2Args& a, int64_t cap_samples, bool uniform, hipStream_t st);
