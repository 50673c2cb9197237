// warp.h - the velocity warp on the host, end to end (warp.hip): which kernel family warps a call's points (warp_kind), which weight images it
// reads in each role (warp_need: a plan takes its rooms from it, the call hands the same bits to vel_images), what a call on the velocity net
// refuses (check_vel_call), and the launches.  The argument blocks of the single kernels (x6.h, pde.h) are filled in warp.hip and nowhere else;
// the launchers - with NVFI_X6W, NVFI_X6W_UNI, NVFI_X6W_MIN_TILES and every ProfScope - stay in the kernels' units.  Host code only.
#pragma once
#include "common.h"
#include "frags.h"
#include "vel.h"

enum WarpKind { WARP_X6, WARP_FP16IN, WARP_FP32 };
// per_point: the no-grad integrators with per-point times (nvfi_integrate_pos, nvfi_compute_alpha, nvfi_render_flow, nvfi_flow_loss_fwd);
// otherwise the render's warp on its uniform step sequence, in training (train) or eval mode.  The table stands beside the definition (warp.hip).
WarpKind warp_kind(const nvfi_field_desc* f, bool train, bool per_point);
// the render plan has room for the fp16 images: a WARP_FP16IN render, and an eval render with vel_fp16 = 3, which has always carried it (pinned sizes)
bool warp_fp16_room(const nvfi_field_desc* f, bool train);
// the training warp writes the z rows of layers 0..3 as x4 stash blocks (x6 forward + fused adjoint, NVFI_RK2_X4): forward and backward both ask here
bool warp_stash_x4(const nvfi_field_desc* f);
// the training render's forward kernel family; its opt-in fp16-input forward (vel_fp16 bit 2) is the render's alone: integrate_pos never takes it
WarpKind advect_kind(const nvfi_field_desc* f);

// the VI_* images (frags.h) a family reads as the per-point warp without gradient, as the forward of a render with nsteps > 0 (the backward asks
// for its transposed images itself) and as the adjoint chain of advect.hip.  A caller that reads more ORs it on (nvfi_render_flow: VI_VEL)
enum WarpRole { WARP_POINTS, WARP_RENDER, WARP_ADJOINT };
unsigned warp_need(WarpKind kind, WarpRole role);

// What a call on the velocity net refuses before anything is launched, error 2 with a message that names the call: check_desc (VEL_CALL_DESC),
// N >= POINTS_PER_CALL_MAX (a call without such a limit passes 0), a field without a velocity net (vW / vb / aW / ab are NULL there: the pack
// kernels would read through them), the fp16-input modes vel_fp16 1 / 2 where they have no adjoint or integrator (VEL_CALL_NO_FP16IN)
enum { VEL_CALL_DESC = 1, VEL_CALL_NO_FP16IN = 2 };
int check_vel_call(const char* who, const nvfi_field_desc* f, int64_t N, unsigned what);

// The per-point warp, no gradient.  count: device count of list entries (NULL: all `cap` points, cap being the launch capacity); list[i] -> point
// index (NULL: identity); xw is updated in place unless xout3 (N,3) is given; pt_t / pt_base are read at the compact index or (pt_by_list) at list[i]
struct WarpPoints {
    const int* count; int64_t cap; const int* list; float4* xw; float* xout3;
    const float* pt_t; const float* pt_base; int pt_by_list; int max_steps;
};
// launch_rk2_x6 / launch_rk2_inf16 / launch_rk2_fwd by kind, on VI's images; img16: the room WARP_FP16IN packs its own image into (2 x PRE16_IMAGE_BYTES)
int warp_points(const nvfi_field_desc* f, WarpKind kind, const VelImages& VI, void* img16, const WarpPoints& p, hipStream_t st);

// The uniform warp.  Its schedule: the host's dts / tcs, the device-side record `sched` (common.h) when that is not NULL, or - pt_dt / pt_tc,
// advect_pt.hip - a device-side table dt[s][i] / tcur[s][i], i the compact index, `cap` apart: every point takes its own steps
struct WarpSchedule { int nsteps; const float* dts; const float* tcs; const float* sched; const float* pt_dt; const float* pt_tc; };
struct WarpStash { float* zst; float* x0st; float* rec; float* gst; int64_t cap_tiles; int z_x4; };   // NULL rooms in eval mode; z_x4: warp_stash_x4
// *ra for the compact list (count, list) of the dense positions xw, cap the launch capacity; gxk: the upstream gradient, the adjoint's alone
void warp_uni_args(const nvfi_field_desc* f, const VelImages& VI, const int* count, const int* list, float4* xw, int64_t cap,
                   const WarpSchedule& s, const WarpStash& stash, const float4* gxk, Rk2Args* ra);
// launch_rk2_x6_uni / launch_rk2_inf16 / launch_rk2_split_uni by kind, `train` writes the stash; with a schedule table the stash-writing _pt forms
int warp_uni_fwd(const nvfi_field_desc* f, WarpKind kind, const VelImages& VI, void* img16, const Rk2Args& ra, bool train, hipStream_t st);
// the unfused adjoint, launch_rk2_split_bwd or its _pt form; gx0: optional (dense, 3) gradient at the starting positions
int warp_uni_bwd(const VelImages& VI, const Rk2Args& ra, float* gx0, hipStream_t st);
