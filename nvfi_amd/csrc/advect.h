// advect.h - the host-side entry to the adjoint chain of integrate_pos that advect.hip (nvfi_advect_grad) and flowloss.hip (nvfi_flow_loss_bwd)
// share: the plan of one chunk of points and the launches behind the caller's own pack kernel.  Host code only: no kernel is declared here.
#pragma once
#include "common.h"
#include "frags.h"
#include "warp.h"

struct AdvectPlan {
    int* count; int* list; float4* xw; float4* gxk;
    float *vel_frag, *vel_x4, *vel_x4b; void* x6img;
    float *slabs, *zst, *x0st, *gst, *rec;
    int64_t cap_tiles, total;
};
// the rooms of a chunk of N points and nsteps RK2 steps in `ws` (NULL: sizes only, P->total); kind: advect_kind(f) (warp.h), whose images
// (warp_need(kind, WARP_ADJOINT)) get a room when the descriptor carries no fragment cache
void plan_advect(const nvfi_field_desc* f, int64_t N, int nsteps, WarpKind kind, void* ws, AdvectPlan* P);
// Behind a pack kernel of the caller's on `st` that has written P.xw (the dense starting positions), P.gxk (the upstream gradient at the
// advected positions), P.list (the identity) and P.count[0] (the DEVICE count of points, <= N): the weight images, the stash-writing uniform
// warp, the unfused adjoint (which stores the gradient at the start into g_x when that is not NULL) and the six weight-gradient jobs,
// ACCUMULATED into grads->vW / vb.  N is the launch capacity; s.nsteps >= 1.
// s: the host's dts / tcs, or (advect_pt.hip) the device-side table s.pt_dt / s.pt_tc - dt[k][i] / tcur[k][i] for k < nsteps and i the index
// in P.list, N apart: every point takes its own steps, one with dt == 0 at a step rests there (the per-point-times kernels of vel_x6.hip /
// vel_split.hip, which warp_uni_fwd / warp_uni_bwd launch for such a schedule).
int advect_chain(const nvfi_field_desc* f, const AdvectPlan& P, int64_t N, const WarpSchedule& s, WarpKind kind, float* g_x,
                 const nvfi_grads* grads, hipStream_t st);
