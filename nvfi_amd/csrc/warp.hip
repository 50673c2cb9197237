// warp.hip - the host side of the velocity warp (warp.h): the kernel-family table, the images each family reads, the refusals of a call on the
// velocity net, and the one place that fills the argument blocks of the warp kernels and calls their launchers.  No kernel is defined here: no
// per-file flags, no packed-fp32 fence.  Reference counterpart: none - integrate_pos (models/tensorf_keyframe.py:575-611) serves every caller.
#include <string.h>
#include "common.h"
#include "warp.h"
#include "pde.h"
#include "render.h"
#include "x6.h"

// ---------------------------------------------------------------- the warp table
// vf = vel_fp16 & 3 (0: default, 1 / 2: the fp16-input modes of pre16.hip, 3: x6 asked for by name); +4: fp16-input forward of the TRAINING
// warp; +8: keep the no-grad integrators on the fp32 MFMA kernel.
//
//                                          vf = 0                                       vf = 1, 2      vf = 3
//   per-point, no grad (integrate_pos,     NVFI_INTEGRATE_X6 (default 1) and no +8:     WARP_FP16IN    WARP_X6      +4 has no say
//   compute_alpha, render_flow, flow_loss) WARP_X6, otherwise WARP_FP32                 (render_flow and flow_loss refuse these two)
//   render, eval                           NVFI_RK2_X6 (default 1): WARP_X6,            WARP_FP16IN    WARP_X6      +4 and +8 have no say
//                                          otherwise WARP_FP32
//   render, train                          +4: WARP_FP16IN; otherwise NVFI_RK2_X6: WARP_X6, else WARP_FP32 - for every vf; +8 has no say
//
// WARP_X6: vel_x6.hip / vel_x6w.hip (fp32 products formed exactly on the 16-bit matrix pipe, tests/test_gpu_x6.py); WARP_FP16IN: pre16.hip; WARP_FP32:
// vel.hip (per point), vel_split.hip (render).  NVFI_RK2_FUSE / NVFI_RK2_X4 choose the adjoint and stash layout behind the forward (warp_stash_x4), not the forward.
WarpKind warp_kind(const nvfi_field_desc* f, bool train, bool per_point) {
    const int vf = f->vel_fp16 & 3;
    if (train) {
        if (f->vel_fp16 & 4) return WARP_FP16IN;
        return sw(NVFI_RK2_X6) ? WARP_X6 : WARP_FP32;
    }
    if (vf == 3) return WARP_X6;
    if (vf != 0) return WARP_FP16IN;
    const bool x6 = per_point ? (sw(NVFI_INTEGRATE_X6) != 0 && !(f->vel_fp16 & 8)) : sw(NVFI_RK2_X6) != 0;
    return x6 ? WARP_X6 : WARP_FP32;
}
bool warp_fp16_room(const nvfi_field_desc* f, bool train) { return warp_kind(f, train, false) == WARP_FP16IN || (!train && (f->vel_fp16 & 3) == 3); }
bool warp_stash_x4(const nvfi_field_desc* f) { return warp_kind(f, true, false) == WARP_X6 && sw(NVFI_RK2_X4) && sw(NVFI_RK2_FUSE); }
WarpKind advect_kind(const nvfi_field_desc* f) {
    const WarpKind k = warp_kind(f, true, false);
    return k == WARP_FP16IN ? (sw(NVFI_RK2_X6) ? WARP_X6 : WARP_FP32) : k;
}

// WARP_FP16IN as a per-point warp reads none of vel_images' (launch_rk2_inf16 packs its own image); advect_kind never asks for its WARP_ADJOINT row
unsigned warp_need(WarpKind kind, WarpRole role) {
    static const unsigned need[3][3] = {          // [role][kind]
        /* WARP_POINTS  */ {VI_X6, 0, VI_VEL},
        /* WARP_RENDER  */ {VI_VEL | VI_X6, VI_VEL, VI_VEL | VI_X4F},
        /* WARP_ADJOINT */ {VI_VEL | VI_X4B | VI_X6, VI_VEL | VI_X4B | VI_X4F, VI_VEL | VI_X4B | VI_X4F}};
    return need[role][kind];
}

int check_vel_call(const char* who, const nvfi_field_desc* f, int64_t N, unsigned what) {
    if ((what & VEL_CALL_DESC) && check_desc(f)) return 2;
    if (N >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "%s: N too large for one call; chunk the points", who);
    if (!f->use_vel) return nvfi_fail(2, "%s needs a field with a velocity net (use_vel = 0)", who);
    const int vf = f->vel_fp16 & 3;
    if ((what & VEL_CALL_NO_FP16IN) && (vf == 1 || vf == 2))
        return nvfi_fail(2, "%s: the fp16-input modes (vel_fp16 = %d) have no adjoint and no flow integrator: use 0, 3 or bit 3", who, f->vel_fp16);
    return 0;
}

int warp_points(const nvfi_field_desc* f, WarpKind kind, const VelImages& VI, void* img16, const WarpPoints& p, hipStream_t st) {
    const int64_t n_direct = p.count ? 0 : p.cap;
    const float dtm = dt_max_of(*f);
    if (kind == WARP_X6) {
        X6Args a; memset(&a, 0, sizeof(a));
        a.f = *f; a.img = VI.x6; a.count = p.count; a.n_direct = n_direct; a.list = p.list; a.xw = p.xw; a.xout3 = p.xout3;
        a.pt_t = p.pt_t; a.pt_base = p.pt_base; a.pt_by_list = p.pt_by_list; a.dt_max = dtm; a.max_steps = p.max_steps;
        return launch_rk2_x6(a, p.cap, st);
    }
    if (kind == WARP_FP16IN) {      // opt-in fp16-input inference mode (pre16.hip); its block has no pt_by_list
        if (p.pt_by_list) return nvfi_fail(2, "the fp16-input integrator reads per-point times at the compact index only");
        Rk16Args h; memset(&h, 0, sizeof(h));
        h.img = img16; h.P = p.cap; h.count = p.count; h.list = p.list; h.xw = p.xw; h.xout = p.xw; h.xout3 = p.xout3;
        h.pt_t = p.pt_t; h.pt_base = p.pt_base; h.dt_max = dtm; h.max_steps = p.max_steps;
        return launch_rk2_inf16(f, h, false, st);
    }
    Rk2Args a; memset(&a, 0, sizeof(a));
    a.f = *f; a.Wv = VI.VW; a.count = p.count; a.n_direct = n_direct; a.list = p.list; a.xw = p.xw; a.xout = p.xout3;
    a.pt_t = p.pt_t; a.pt_base = p.pt_base; a.pt_by_list = p.pt_by_list; a.dt_max = dtm; a.max_steps = p.max_steps;
    return launch_rk2_fwd(a, p.cap, false, st);
}

void warp_uni_args(const nvfi_field_desc* f, const VelImages& VI, const int* count, const int* list, float4* xw, int64_t cap,
                   const WarpSchedule& s, const WarpStash& stash, const float4* gxk, Rk2Args* ra) {
    memset(ra, 0, sizeof(*ra));
    ra->f = *f; ra->Wv = VI.VW; ra->count = count; ra->list = list; ra->xw = xw;
    ra->nsteps = s.nsteps; ra->sched = s.sched;
    if (s.pt_dt) { ra->pt_t = s.pt_dt; ra->pt_base = s.pt_tc; }
    else for (int k = 0; k < s.nsteps; ++k) { ra->dt[k] = s.dts[k]; ra->tcur[k] = s.tcs[k]; }
    ra->zst = stash.zst; ra->x0st = stash.x0st; ra->rec = stash.rec; ra->gst = stash.gst; ra->cap = cap; ra->cap_tiles = stash.cap_tiles;
    ra->z_x4 = stash.z_x4; ra->gxk = gxk;
}

int warp_uni_fwd(const nvfi_field_desc* f, WarpKind kind, const VelImages& VI, void* img16, const Rk2Args& ra, bool train, hipStream_t st) {
    const bool pt = ra.pt_t != nullptr;        // (the uniform kernels read no per-point times: the pointer means the schedule table)
    if (kind == WARP_X6) {      // vel_x6.hip: fp32 products formed exactly from three bfloat16 terms per operand; same stash / records for the fp32 adjoint
        X6UniArgs a; a.r = ra; a.img = VI.x6;
        return pt ? launch_rk2_x6_uni_pt(a, ra.cap, st) : launch_rk2_x6_uni(a, ra.cap, train, st);
    }
    if (kind == WARP_FP16IN) {
        // opt-in fp16-input modes (pre16.hip): eval-mode renders (vel_fp16 bits 0-1), and - bit 2 - the FORWARD of a training render's warp, which
        // writes the same stash as k_rk2_split_uni<STASH> (the adjoint and the weight gradients stay fp32 MFMA)
        if (pt) return nvfi_fail(2, "the fp16-input warp has no per-point-times form");
        Rk16Args h; memset(&h, 0, sizeof(h));
        h.img = img16; h.P = ra.cap; h.count = ra.count; h.list = ra.list; h.xw = ra.xw; h.xout = ra.xw; h.nsteps = ra.nsteps; h.sched = ra.sched;
        h.zst = ra.zst; h.x0st = ra.x0st; h.rec = ra.rec; h.cap = ra.cap; h.cap_tiles = ra.cap_tiles;
        for (int k = 0; k < ra.nsteps; ++k) { h.dt[k] = ra.dt[k]; h.tcur[k] = ra.tcur[k]; }
        return launch_rk2_inf16(f, h, true, st, train);
    }
    // fp32: the feature-split layout of vel_split.hip (the one-tile-per-wave k_rk2_fwd<uniform> of vel.hip, NVFI_RK2_SPLIT=0 - same stash, same
    // numbers bit for bit - was retired in round 6)
    SplitUniArgs a; a.r = ra;
    for (int l = 0; l < 6; ++l) { a.f4[l] = VI.f4[l]; a.bv[l] = VI.VW.b[l]; }
    return pt ? launch_rk2_split_uni_pt(a, ra.cap, st) : launch_rk2_split_uni(a, ra.cap, train, st);
}

// vel_split.hip (k_rk2_bwd of vel.hip, NVFI_RK2_SPLIT_BWD=0 - the same adjoint stash bit for bit - was retired in round 6)
int warp_uni_bwd(const VelImages& VI, const Rk2Args& ra, float* gx0, hipStream_t st) {
    SplitBwdArgs a; a.r = ra; a.gx0 = gx0;
    for (int l = 0; l < 6; ++l) a.t4[l] = VI.t4[l];
    return ra.pt_t ? launch_rk2_split_bwd_pt(a, ra.cap, st) : launch_rk2_split_bwd(a, ra.cap, st, gx0 != nullptr);
}
