// render.hip - ray marching through the keyframe K-plane field, host side: the workspace plan, the forward (sampling, velocity warp,
// density gather, volume weights, appearance MLP, composite) and the hand-written backward of all of it.  The kernels are the units'
// named in render.h.  Reference semantics: models/tensorf_keyframe.py:641-755 (render_pts), 575-609 (the warp's schedule).
//
// Work decomposition (MI355X-first): the reference's boolean-mask gather/scatter with a host sync
// per mask becomes on-device compaction (per-ray counts -> one-block scan -> ordered fill), so no
// kernel launch depends on a host-visible count.  Gathers read channel-last planes with 16-byte
// loads; per-ray scans/reductions are wave-level; the MLP contractions run on the MFMA engine.
#include "common.h"
#include "render.h"
#include "fuse.h"
#include "pde.h"
#include "warp.h"
#include "x6.h"

// The warp's kernel family (warp_kind), its images, its launches (warp_uni_*) and what the family means for the training stash (warp_stash_x4)
// are warp.h's; the fused adjoint (launch_rk2_fuse_bwd) is launched here on the same Rk2Args.  NVFI_RK2_X6 (default 1): the x6
// kernels; NVFI_RK2_FUSE (default 1): the adjoint + hidden-layer weight gradients in one persistent kernel - then the z rows of layers 0..3 have
// ONE reader and travel as x4 stash blocks (a quarter of the stash instructions on both sides; NVFI_RK2_X4=0: row-major)

// Optional side stream for the plane-gradient scatters (NVFI_SIDE_STREAM=1): they are bound by L2 atomics and leave the MFMA
// pipes idle, so the backward can fork them next to the weight-gradient / RK2-adjoint kernels and join before returning.
// Off by default: it gained 2.5 % while those kernels ran two workgroups per CU, but since they own a CU each (one wave per
// SIMD with the whole register file, engine.h: FragPipe) a scatter wave cannot co-reside with them and the fork only splits CUs.
// NVFI_BWD_FORK (flags bit 16), for a caller that drives ONE stream: parts of the render backward run on a library-owned stream, with their
// own tile-sort workspace / slab region, joined before the call returns.
//   keyframe time: the two halves - appearance (k_app_bwd, k_og<48>, tile scatter, render-MLP weight gradients) and density (k_weights_bwd,
//     k_og<24>, tile scatter) - share nothing but inputs: the density half runs beside the appearance half;
//   non-keyframe time: the coordinate gradients chain k_app_bwd -> k_og<48> -> k_og<24> -> RK2 adjoint -> velocity-net weight gradients; the
//     plane scatters of both branches and the render-MLP weight gradients hang off that chain and run beside it.
// A caller that already overlaps several renders / the PDE term on its own streams (bench.py's fused driver) leaves the bit off.
// Both are library-owned streams with their fork / join events, one set per device ordinal: a second device (or a second field on another
// device) in the same process gets its own instead of launching its forked half on the first device's.  Created on the first call on the
// device (autograd runs backward nodes on per-device worker threads); a creation that fails is remembered and leaves the caller on one stream.
struct LibStream { hipStream_t s; hipEvent_t fork[2], join; bool ok; };
static PerDevice<LibStream> g_sides, g_forks;
static LibStream* lib_stream(PerDevice<LibStream>& per) {
    LibStream* l = per.get([](LibStream& n, int) {
        n.ok = hipStreamCreateWithFlags(&n.s, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&n.fork[0], hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&n.fork[1], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&n.join, hipEventDisableTiming) == hipSuccess;
        return 0;
    });
    return l->ok ? l : nullptr;
}

// NVFI_DETERMINISTIC=1: bit-reproducible plane gradients for tests.  The sorted-tile path sums in an order that
// depends on atomic cursors; this mode takes the plain atomic scatter instead and accumulates in fixed point (k_plane_scatter<C, true>).
static bool det_mode() { return sw(NVFI_DETERMINISTIC) != 0; }
// ================================================================ host: fragment jobs, launches, ABI
int pack_render_frags(const nvfi_field_desc* f, float* buf, RenderFrags* out, PackJobs* jobs) {
    float* p = buf;
    auto take = [&](int n) { float* r = p; p += n; return r; };
    float* fb = take(RF_B); float* f1 = take(RF_1); float* f2 = take(RF_2); float* f3 = take(RF_3);
    float* b1 = take(128); float* b2 = take(128); float* b3 = take(32);
    float* t3 = take(RT_3); float* t2 = take(RT_2); float* t1 = take(RT_1); float* tb = take(RT_B);
    auto add = [&](const float* W, const float* b, float* frag, float* bfrag, int o, int in, int MT, int NS, int rk, int sk, int tr) {
        if (jobs->n >= MAX_PACK_JOBS) return 1;
        PackJob& J = jobs->j[jobs->n++];
        J.W = W; J.b = b; J.frag = frag; J.bfrag = bfrag; J.out = o; J.in = in; J.MT = MT; J.NS = NS;
        J.row_kind = rk; J.slot_kind = sk; J.transposed = tr; J.x4 = 0;
        return 0;
    };
    int rc = 0;
    rc |= add(f->basis, nullptr, fb, nullptr, f->app_dim, f->Ca, 1, 24, RK_NATURAL, SK_HIDDEN, 0);
    if (f->shading == 0) {      // SH shading has no render MLP (tensorf_base.py:196-197)
        rc |= add(f->rW[0], f->rb[0], f1, b1, 128, 110, 4, 55, RK_NATURAL, SK_RENDER_IN, 0);
        rc |= add(f->rW[1], f->rb[1], f2, b2, 128, 128, 4, 64, RK_NATURAL, SK_HIDDEN, 0);
        rc |= add(f->rW[2], f->rb[2], f3, b3, 3, 128, 1, 64, RK_NATURAL, SK_HIDDEN, 0);
        rc |= add(f->rW[2], nullptr, t3, nullptr, 3, 128, 4, 4, RK_NATURAL, SK_HIDDEN, 1);
        rc |= add(f->rW[1], nullptr, t2, nullptr, 128, 128, 4, 64, RK_NATURAL, SK_HIDDEN, 1);
        rc |= add(f->rW[0], nullptr, t1, nullptr, 128, 110, 4, 64, RK_RENDER_IN, SK_HIDDEN, 1);
    }
    rc |= add(f->basis, nullptr, tb, nullptr, f->app_dim, f->Ca, 2, 16, RK_NATURAL, SK_HIDDEN, 1);
    if (rc) return nvfi_fail(3, "too many pack jobs");
    out->fb = fb; out->f1 = f1; out->b1 = b1; out->f2 = f2; out->b2 = b2; out->f3 = f3; out->b3 = b3;
    out->t3 = t3; out->t2 = t2; out->t1 = t1; out->tb = tb;
    return 0;
}

int check_desc(const nvfi_field_desc* f) {
    if (f->Cd != 24 || f->Ca != 48 || f->app_dim != (f->shading == 1 ? 27 : 32) || f->shading < 0 || f->shading > 1)
        return nvfi_fail(2, "unsupported component counts Cd=%d Ca=%d app_dim=%d shading=%d (kernels are built for 24/48/32 with MLP_PE, 24/48/27 with SH)", f->Cd, f->Ca, f->app_dim, f->shading);
    if (f->n_samples < 1 || f->n_samples > 1024) return nvfi_fail(2, "n_samples=%d outside [1,1024]", f->n_samples);
    return 0;
}

#define NSLAB_MAX 256        // (1024 while NVFI_NSLAB could be swept: 0.6 GB of slab workspace nobody wrote)
#define NSLAB 256            // slab capacity of a weight-gradient job (one per CU; the NVFI_NSLAB sweep of round 2 was retired in round 6)
#define SLAB_FLOATS (128 * 128 + 128)

static void plan_render(const nvfi_field_desc* f, int64_t R, int flags, int nsteps, void* ws, RenderPlan* P) {
    Bump B{(char*)ws, 0, 0};
    const int64_t N = R * f->n_samples;
    const bool train = flags & NVFI_TRAIN;
    P->N = N; P->nsteps = nsteps;
    P->cap_tiles = (N + WG_SAMPLES - 1) / WG_SAMPLES * 4;   // whole workgroups: every wave of an active workgroup owns a stash tile
    const int64_t off_counters = align_up(B.off, 256);
    P->counters = B.take<int>(16);
    // the histograms (+ tickets) of the backward's two counting sorts sit right behind the counters: the forward's one fill zeroes all
    // three (the scans re-zero the histograms after every use, so the backward needs no fill of its own)
    P->tiles = train && tile_geom(f, &P->tw.g) == 0 && sw(NVFI_SCATTER_TILES) && !det_mode();
    P->tw.hist = P->tw2.hist = nullptr;
    if (P->tiles) { P->tw2.g = P->tw.g; P->tw.hist = B.take<int>(P->tw.g.nbins + 64); P->tw2.hist = B.take<int>(P->tw.g.nbins + 64); }
    // ... and so do the look-back words of the two fused compactions (k_sample_fill, k_weights_fill): one per workgroup of 4 rays
    const int64_t ray_wgs = (R + 3) / 4;
    P->lb_s = B.take<unsigned long long>(ray_wgs); P->lb_w = B.take<unsigned long long>(ray_wgs);
    P->mse_part = B.take<float>(ray_wgs);        // nvfi_render_fwd_mse: per-workgroup partial sums of k_final_fwd (ticket: counters[8])
    P->zero_bytes = align_up(B.off, 256) - off_counters;
    P->sched = B.take<float>(SCHED_FLOATS);
    P->cnt_v = B.take<int>(R); P->off_v = B.take<int>(R + 1);
    P->cnt_m = B.take<int>(R); P->off_m = B.take<int>(R + 1);
    P->vlist = B.take<int>(N); P->mlist = B.take<int>(N);
    P->valid = B.take<uint8_t>(N); P->mflag = B.take<uint8_t>(N);
    P->cnt_r = P->off_r = P->rlist = nullptr; P->rflag = nullptr;
    if (nsteps > 0) { P->cnt_r = B.take<int>(R); P->off_r = B.take<int>(R + 1); P->rlist = B.take<int>(N); P->rflag = B.take<uint8_t>(N); }
    P->xw = B.take<float4>(N + 1); P->rgbs = B.take<float4>(N); P->rgb_pre = B.take<float4>(R);
    P->xpre = B.take<float>(N);
    P->vel_frag = B.take<float>(VEL_FRAG_FLOATS);
    P->vel_x4 = nsteps > 0 ? B.take<float>(VEL_X4F_FLOATS) : nullptr;
    P->img16 = (nsteps > 0 && warp_fp16_room(f, train)) ? (void*)B.take<float4>(2 * PRE16_IMAGE_BYTES / 16) : nullptr;   // fp16 images (hi, lo)
    P->vel_x4b = (nsteps > 0 && train) ? B.take<float>(VEL_X4B_FLOATS) : nullptr;
    P->x6img = nsteps > 0 ? (void*)B.take<float>(X6_IMAGE_BYTES / 4) : nullptr;      // the x6 images when the descriptor carries no fragment cache
    P->x6imgT = (nsteps > 0 && train) ? (void*)B.take<float>(X6_IMAGE_BYTES / 4) : nullptr;      // ... and their transposes (the adjoint's dgrad, vel_fuse.hip)
    P->render_frag = B.take<float>(RENDER_FRAG_FLOATS);
    P->maskv = (flags & NVFI_WANT_MASK) ? B.take<float>(N * 32) : nullptr;
    P->mask_frag = (flags & NVFI_WANT_MASK) ? B.take<float>(64 * 1024) : nullptr;
    P->app_relu = nullptr;
    P->app_f = P->app_b = P->zst = P->x0st = P->rec = P->gst = P->slabs = nullptr;
    P->gxw = P->gxk = nullptr; P->gxpre = nullptr; P->gg = nullptr;
    if (train) {
        P->gxw = B.take<float4>(N); P->gxk = B.take<float4>(N); P->gxpre = B.take<float>(N);
        P->gg = B.take<float>(N * 48);
        P->app_f = B.take<float>(P->cap_tiles * (int64_t)(APP_F_ROWS * REGF));
        P->app_b = B.take<float>(P->cap_tiles * (int64_t)(APP_B_ROWS * REGF));
        P->app_relu = B.take<unsigned>(P->cap_tiles * (int64_t)256);
        P->slabs = B.take<float>((int64_t)NSLAB_MAX * SLAB_FLOATS * 6);
        P->shadow = nullptr;
        if (det_mode()) { int64_t off[12]; P->shadow = B.take<long long>(plane_elems(f, off)); }
        if (P->tiles) plan_tile_scatter(B, f, N, &P->tw);
        if (P->tiles) plan_tile_scatter(B, f, N, &P->tw2);     // NVFI_BWD_FORK: the density half of the backward sorts / scatters beside the appearance half
        P->slabs2 = nsteps > 0 ? B.take<float>((int64_t)NSLAB_MAX * SLAB_FLOATS * 6) : nullptr;   // ... and the velocity-net slabs beside the render-MLP slabs
        if (nsteps > 0) {
            const int64_t nev = 2 * (int64_t)nsteps;
            P->zst = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_Z_REGS * REGF));
            P->x0st = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_X0_REGS * REGF));
            P->gst = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_G_REGS * REGF));
            P->rec = B.take<float>((int64_t)nsteps * RK_NF * N);
        }
    }
    // flow branch (inference, flow.hip): compacted (x, t) of the masked samples, their displaced positions, their gated velocities, the per-point
    // base times of the integrator and its own x6 image (a keyframe render plans none).  Last, so that the flag moves nothing in front of it
    P->flow_xt = P->flow_xd = P->flow_vg = nullptr; P->flow_tb = P->flow_x6 = nullptr;
    if ((flags & NVFI_WANT_FLOW) && !train) {
        P->flow_xt = B.take<float4>(N); P->flow_xd = B.take<float4>(N); P->flow_vg = B.take<float4>(N);
        P->flow_tb = B.take<float>(2 * N); P->flow_x6 = B.take<float>(X6_IMAGE_BYTES / 4);
    }
    // object-selected render (inference, objects.hip): one float per sample and the packed MaskField.  Behind the flow room: moves nothing either
    P->sel = P->sel_frag = nullptr;
    if ((flags & NVFI_WANT_SELECT) && !train) { P->sel = B.take<float>(N); P->sel_frag = B.take<float>(64 * 1024); }
    P->total = align_up(B.off, 256);
}

int render_plan_at(const nvfi_field_desc* f, int64_t R, int flags, float t, void* ws, int64_t ws_bytes, RenderPlan* P, float* base, float* dts, float* tcs) {
    if (check_desc(f)) return 2;
    float base_[1], dts_[MAX_RK_STEPS], tcs_[MAX_RK_STEPS];
    const int nsteps = rk_schedule(*f, t, flags, base ? base : base_, dts ? dts : dts_, tcs ? tcs : tcs_);
    if (nsteps < 0) return nvfi_fail(2, "t=%g needs more than %d RK2 steps", t, MAX_RK_STEPS);
    plan_render(f, R, flags, nsteps, ws, P);
    if (ws && P->total > ws_bytes) return nvfi_fail(4, "workspace too small: need %lld bytes, got %lld", (long long)P->total, (long long)ws_bytes);
    return 0;
}

extern "C" int nvfi_render_workspace_bytes(const nvfi_field_desc* f, int64_t R, int flags, int64_t* bytes) {
    if (check_desc(f)) return 2;
    // t-independent upper bound: a training call may need up to 2 RK2 steps (|t-base| <= dt_max up to
    // rounding); extrapolated times need more and are re-planned by the caller via nvfi_render_workspace_bytes_t.
    RenderPlan P;
    plan_render(f, R, flags, (f->use_vel && (flags & NVFI_TRAIN)) ? 2 : 0, nullptr, &P);
    *bytes = P.total;
    return 0;
}
extern "C" int nvfi_render_workspace_bytes_t(const nvfi_field_desc* f, int64_t R, int flags, float t, int64_t* bytes) {
    RenderPlan P;
    if (int rc = render_plan_at(f, R, flags, t, nullptr, 0, &P)) return rc;
    *bytes = P.total;
    return 0;
}

// what only some of the forward's entry points pass.  target / loss_scale / loss / g_rgb: nvfi_render_fwd_mse; sel_m / select: nvfi_render_fwd_select
struct FwdExtras {
    const float* target = nullptr; float loss_scale = 1.f; float* loss = nullptr; float* g_rgb = nullptr;
    const nvfi_mask_desc* sel_m = nullptr; const float* select = nullptr;
};
static int render_fwd_impl(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d,
                           const float* jitter, float t, const float* t_dev, int flags, float* rgb, float* depth, float* acc,
                           float* weights, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream, const FwdExtras& x = FwdExtras()) {
    hipStream_t st = (hipStream_t)stream;
    if (check_desc(f)) return 2;
    if (R <= 0) return 0;
    if (R * (int64_t)f->n_samples >= (1ll << 31) - 64) return nvfi_fail(2, "R*S too large for one call; chunk the rays");
    if (ensure_scatter_attrs() || ensure_lds_attrs()) return 1;
    const bool train = flags & NVFI_TRAIN;
    float base, dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    RenderPlan P;
    if (int rc = render_plan_at(f, R, flags, t, workspace, workspace_bytes, &P, &base, dts, tcs)) return rc;
    const int S = f->n_samples, nsteps = P.nsteps;
    const int64_t N = P.N;
    const float tn = f->use_vel ? norm_time(*f, base) : norm_time(*f, t);
    const bool fl = sw(NVFI_FUSED_LAUNCH) != 0;
    if (t_dev && nsteps > 4) return nvfi_fail(2, "a device-side time supports plans of up to 4 RK2 steps (t=%g needs %d)", t, nsteps);
    const float* sched = t_dev ? P.sched : nullptr;
    // head: clear of the counters / histograms / look-back words, the device-side schedule (from the host's plan) and the origin test
    SchedArgs sc; memset(&sc, 0, sizeof(sc));
    sc.f = *f; sc.t_dev = t_dev; sc.flags = flags; sc.nsteps_plan = nsteps; sc.tn_plan = tn; sc.sched = P.sched;
    for (int s = 0; s < nsteps && s < 4; ++s) { sc.dt_plan[s] = dts[s]; sc.tc_plan[s] = tcs[s]; }
    if (launch_ray_head(sc, R, rays_o, P.counters, P.zero_bytes, P.counters + 2, fl, st)) return 1;
    // fragments (weights change every optimiser step: repack per call, ~0.3 MB)
    // (round 5: or not at all - a descriptor that carries the field's fragment cache, nvfi_pack_frags, points the kernels at it)
    // the velocity net's images of the warp's kernel come from vel_images (frags.h); the render MLP's pack jobs ride in its k_pack launch
    PackJobs jobs; jobs.n = 0;
    RenderFrags RW; VelImages VI;
    if (pack_render_frags(f, render_frag_room(f, P.render_frag), &RW, &jobs)) return 3;
    const WarpKind kind = warp_kind(f, train, false);
    if (int rc = vel_images(f, nsteps > 0 ? warp_need(kind, WARP_RENDER) : 0,VelImageRoom{P.vel_frag, nullptr, P.vel_x4, P.vel_x4b, nullptr, P.x6img, P.x6imgT}, &VI, &jobs, 0, st)) return rc;
    // sampling; second compact list (nsteps > 0): the valid samples inside the velocity gate (counters[3])
    SampleArgs sa; memset(&sa, 0, sizeof(sa));
    sa.f = *f; sa.R = R; sa.o = rays_o; sa.d = rays_d; sa.u = jitter; sa.train = train; sa.inside = P.counters + 2;
    sa.xw = P.xw; sa.xpre = P.xpre; sa.valid = P.valid; sa.cnt = P.cnt_v; sa.rflag = P.rflag; sa.cnt_r = P.cnt_r;
    sa.lb = P.lb_s; sa.vlist = P.vlist; sa.rlist = P.rlist; sa.total_v = P.counters + 0; sa.total_r = P.counters + 3;
    if (launch_sample(sa, P.off_v, P.off_r, fl, st)) return 1;
    // velocity warp back to the keyframe
    if (nsteps > 0) {
        Rk2Args ra;
        warp_uni_args(f, VI, P.counters + 3, P.rlist, P.xw, N, WarpSchedule{nsteps, dts, tcs, sched, nullptr, nullptr},
                      WarpStash{P.zst, P.x0st, P.rec, P.gst, P.cap_tiles, (train && warp_stash_x4(f)) ? 1 : 0}, nullptr, &ra);
        if (warp_uni_fwd(f, kind, VI, P.img16, ra, train, st)) return 1;
    }
    // density
    DensityArgs da; memset(&da, 0, sizeof(da));
    da.f = *f; da.count = P.counters + 0; da.list = P.vlist; da.xw = P.xw; da.xpre = P.xpre; da.tn = tn; da.sched = sched;
    { ProfScope ps(PK_DENSITY_FWD, st); if (launch_density_q(da, N, st)) return 1; }
    // weights
    WeightArgs wa; memset(&wa, 0, sizeof(wa));
    wa.R = R; wa.S = S; wa.xpre = P.xpre; wa.xw = P.xw; wa.distance_scale = f->distance_scale; wa.weight_thres = f->weight_thres;
    wa.far_ = f->far_; wa.weight = weights; wa.mflag = P.mflag; wa.acc = acc; wa.depth = depth; wa.cnt_m = P.cnt_m;
    wa.lb = P.lb_w; wa.off_m_out = P.off_m; wa.mlist = P.mlist; wa.total_m = P.counters + 1;
    if (x.select) {   // object selection: the MaskField over the valid list, one float per sample; the weights kernels multiply sigma by it
        if (launch_select(x.sel_m, x.select, P.counters + 0, P.vlist, P.xw, P.sel, P.sel_frag, N, st)) return 1;
        wa.sel = P.sel;
    }
    if (launch_weights_fwd(wa, fl, st)) return 1;
    // appearance
    AppArgs aa; memset(&aa, 0, sizeof(aa));
    aa.f = *f; aa.W = RW; aa.count = P.counters + 1; aa.list = P.mlist; aa.xw = P.xw; aa.tn = tn; aa.S = S; aa.sched = sched;
    aa.rays_d = rays_d; aa.rgbs = P.rgbs; aa.stash_f = P.app_f; aa.relu_mask = P.app_relu;
    {
        ProfScope ps(PK_APP_FWD, st);
        // train: the plane-product features of the masked samples from their own gather kernel (parked in gg, which only the backward writes)
        if (train && f->Ca == 48) {
            OgArgs oa; memset(&oa, 0, sizeof(oa));
            oa.f = *f; oa.count = P.counters + 1; oa.list = P.mlist; oa.xw = P.xw; oa.tn = tn; oa.sched = sched; oa.og = P.gg;
            if (launch_app_feat(oa, N, st)) return 1;
            aa.feat48 = P.gg;
        }
        if (launch_app_fwd(aa, N, train, st)) return 1;
    }
    // composite
    FinalArgs fa; fa.R = R; fa.off_m = P.off_m; fa.mlist = P.mlist; fa.weight = weights; fa.rgbs = P.rgbs; fa.acc = acc;
    fa.white_bg = (flags & NVFI_WHITE_BG) ? 1 : 0; fa.rgb_pre = P.rgb_pre; fa.rgb = rgb;
    fa.c = P.counters; fa.nsteps = nsteps; fa.sched = sched;
    fa.target = x.target; fa.g_rgb_out = x.g_rgb; fa.loss_out = x.loss; fa.partial = P.mse_part; fa.ticket = P.counters + 8; fa.loss_scale = x.loss_scale;
    return launch_final_fwd(fa, counters, fl, st);
}


extern "C" int nvfi_render_fwd(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d,
                               const float* jitter, float t, int flags, float* rgb, float* depth, float* acc,
                               float* weights, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream) {
    return nvfi_render_fwd_t(f, R, rays_o, rays_d, jitter, t, nullptr, flags, rgb, depth, acc, weights, workspace, workspace_bytes, counters, stream);
}

// nvfi_render_fwd with the density of every valid sample scaled by s(x) = sum_k select_k softmax(MaskField(x))_k before the weights (objects.hip)
extern "C" int nvfi_render_fwd_select(const nvfi_field_desc* f, const nvfi_mask_desc* m, const float* select, int64_t R, const float* rays_o,
                                      const float* rays_d, const float* jitter, float t, int flags, float* rgb, float* depth, float* acc,
                                      float* weights, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream) {
    if (!select) return nvfi_render_fwd(f, R, rays_o, rays_d, jitter, t, flags, rgb, depth, acc, weights, workspace, workspace_bytes, counters, stream);
    if (flags & NVFI_TRAIN) return nvfi_fail(2, "nvfi_render_fwd_select is an inference call: NVFI_TRAIN renders have no object selection");
    if (!(flags & NVFI_WANT_SELECT)) return nvfi_fail(2, "nvfi_render_fwd_select needs a workspace planned with NVFI_WANT_SELECT in flags");
    if (!m) return nvfi_fail(2, "nvfi_render_fwd_select needs a mask field descriptor");
    FwdExtras x; x.sel_m = m; x.select = select;
    return render_fwd_impl(f, R, rays_o, rays_d, jitter, t, nullptr, flags, rgb, depth, acc, weights, workspace, workspace_bytes, counters, stream, x);
}
extern "C" int nvfi_render_fwd_t(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d,
                                 const float* jitter, float t, const float* t_dev, int flags, float* rgb, float* depth, float* acc,
                                 float* weights, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream) {
    return render_fwd_impl(f, R, rays_o, rays_d, jitter, t, t_dev, flags, rgb, depth, acc, weights, workspace, workspace_bytes, counters, stream);
}
extern "C" int nvfi_render_fwd_mse(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d,
                                   const float* jitter, float t, const float* t_dev, int flags, float* rgb, float* depth, float* acc,
                                   float* weights, void* workspace, int64_t workspace_bytes, int64_t* counters,
                                   const float* target, float loss_scale, float* loss, float* g_rgb, void* stream) {
    if (!target || !loss || !g_rgb) return nvfi_fail(2, "nvfi_render_fwd_mse: target, loss and g_rgb must be non-NULL");
    FwdExtras x; x.target = target; x.loss_scale = loss_scale; x.loss = loss; x.g_rgb = g_rgb;
    return render_fwd_impl(f, R, rays_o, rays_d, jitter, t, t_dev, flags, rgb, depth, acc, weights, workspace, workspace_bytes, counters, stream, x);
}

extern "C" int nvfi_render_bwd(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t,
                               int flags, const float* weights, const float* g_rgb, const float* g_depth,
                               const float* g_acc, const float* g_weights, const nvfi_grads* grads, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    return nvfi_render_bwd_t(f, R, rays_o, rays_d, t, 0, flags, weights, g_rgb, g_depth, g_acc, g_weights, grads, workspace, workspace_bytes, stream);
}

extern "C" int nvfi_render_bwd_t(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t, int t_on_device,
                                 int flags, const float* weights, const float* g_rgb, const float* g_depth,
                                 const float* g_acc, const float* g_weights, const nvfi_grads* grads, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (check_desc(f)) return 2;
    if (R <= 0) return 0;
    if (!(flags & NVFI_TRAIN)) return nvfi_fail(2, "nvfi_render_bwd needs the workspace of a NVFI_TRAIN forward");
    if (ensure_scatter_attrs() || ensure_lds_attrs()) return 1;
    float base, dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    RenderPlan P;
    if (int rc = render_plan_at(f, R, flags, t, workspace, workspace_bytes, &P, &base, dts, tcs)) return rc;
    const int S = f->n_samples, nsteps = P.nsteps;
    const int64_t N = P.N;
    const float tn = f->use_vel ? norm_time(*f, base) : norm_time(*f, t);
    const float* sched = t_on_device ? P.sched : nullptr;     // the record the forward's k_sched left in the workspace
    LibStream* const sides = sw(NVFI_SIDE_STREAM) ? lib_stream(g_sides) : nullptr;
    const bool side = sides && !P.tiles && !det_mode();        // the tile scatter reuses one og buffer for both branches: same stream
    const bool want_aplanes0 = grads->aps[0] || grads->apt[0], want_dplanes0 = grads->dps[0] || grads->dpt[0];
    LibStream* const forks = ((flags & NVFI_BWD_FORK) && P.tiles && want_aplanes0 && want_dplanes0 && !det_mode()) ? lib_stream(g_forks) : nullptr;
    const bool forkable = forks != nullptr;
    const bool fork = forkable && nsteps == 0, fork2 = forkable && nsteps > 0;
    hipStream_t sd = st;                                     // stream of k_weights_bwd / k_og<24> (keyframe fork: the side stream)
    hipStream_t s_atail = st, s_dtail = st;                  // streams of the appearance tail (scatter, render-MLP weight gradients) and of the density scatter
    if (fork) { sd = forks->s; s_dtail = forks->s; }
    if (fork2) { s_atail = forks->s; s_dtail = forks->s; }
    // round 5: both counting sorts of the backward (masked list -> P.tw, valid list -> P.tw2) in ONE pair of launches, up front - the lists and the
    // positions are the forward's; the density branch then always sorts into tw2 and keeps sharing the og buffer unless it runs on the side stream
    const bool fl = sw(NVFI_FUSED_LAUNCH) != 0;
    const bool want_asort = P.tiles && want_aplanes0, want_dsort = P.tiles && want_dplanes0;
    const bool presort = fl && (want_asort || want_dsort);
    TileWork twd_v = (fork || fork2 || presort) ? P.tw2 : P.tw;
    if (presort && !(fork || fork2)) twd_v.og = P.tw.og;
    const TileWork& twd = twd_v;
    if (presort) {
        const TileWork* wp[2]; const int* cp[2]; const int* lp[2]; int nj = 0;
        if (want_asort) { wp[nj] = &P.tw; cp[nj] = P.counters + 1; lp[nj] = P.mlist; ++nj; }
        if (want_dsort) { wp[nj] = &twd; cp[nj] = P.counters + 0; lp[nj] = P.vlist; ++nj; }
        ProfScope ps(PK_DENSITY_SCATTER, st);
        if (launch_tile_sort(wp, cp, lp, nj, P.xw, N, st)) return 1;
    }
    if (fork) { HIPCK(hipEventRecord(forks->fork[0], st)); HIPCK(hipStreamWaitEvent(forks->s, forks->fork[0], 0)); }     // (behind the sorts)
    // deterministic mode: the scatters add fixed-point integers into int64 shadow planes; k_det_finish folds them into the gradients
    nvfi_grads gdet = *grads;
    if (det_mode()) {
        int64_t det_off[12];
        const int64_t det_n = plane_elems(f, det_off);
        if (launch_zero(P.shadow, det_n * (int64_t)sizeof(long long), st)) return 1;
        for (int i = 0; i < 3; ++i) {
            if (gdet.dps[i]) gdet.dps[i] = reinterpret_cast<float*>(P.shadow + det_off[i]);
            if (gdet.dpt[i]) gdet.dpt[i] = reinterpret_cast<float*>(P.shadow + det_off[3 + i]);
            if (gdet.aps[i]) gdet.aps[i] = reinterpret_cast<float*>(P.shadow + det_off[6 + i]);
            if (gdet.apt[i]) gdet.apt[i] = reinterpret_cast<float*>(P.shadow + det_off[9 + i]);
        }
    }
    // the plain fragments were packed by the forward into the same workspace (... or live in the field's fragment cache: the same weights, the
    // caller's contract); the adjoint's own images - x4 transposed copies, and the transposed x6 image of the fused kernel - are packed here
    RenderFrags RW; PackJobs unused; unused.n = 0;
    pack_render_frags(f, render_frag_room(f, P.render_frag), &RW, &unused);
    const int fuse = sw(NVFI_RK2_FUSE) ? 1 : 0;
    VelImages VI;
    if (int rc = vel_images(f, nsteps > 0 ? (VI_VEL | VI_X4B | (fuse ? VI_X6T : 0)) : 0, VelImageRoom{P.vel_frag, nullptr, P.vel_x4, P.vel_x4b, nullptr, P.x6img, P.x6imgT},
                            &VI, nullptr, VI_VEL, st)) return rc;
    bool forked = false;
    // appearance branch
    AppArgs aa; memset(&aa, 0, sizeof(aa));
    aa.f = *f; aa.W = RW; aa.count = P.counters + 1; aa.list = P.mlist; aa.xw = P.xw; aa.tn = tn; aa.S = S; aa.sched = sched;
    aa.rays_d = rays_d; aa.rgbs = P.rgbs; aa.stash_f = P.app_f; aa.relu_mask = P.app_relu; aa.stash_b = P.app_b; aa.g = *grads;
    aa.g_rgb = g_rgb; aa.rgb_pre = P.rgb_pre; aa.weight = weights; aa.gxw = P.gxw; aa.gg = P.gg;
    aa.plane_tail = P.tiles ? 0 : 1;
    { ProfScope ps(PK_APP_BWD, st); if (launch_app_bwd(aa, N, st)) return 1; }
    const bool want_aplanes = grads->aps[0] || grads->apt[0];
    if (P.tiles) {
        if (want_aplanes || nsteps > 0) {
            // one pass over the masked samples: per-plane value gradients (og) for the tile scatter and, at non-keyframe times,
            // the plane part of the coordinate gradients (they only feed the RK2 adjoint)
            ProfScope ps(PK_APP_SCATTER, st);
            OgArgs oa; memset(&oa, 0, sizeof(oa));
            oa.f = *f; oa.count = P.counters + 1; oa.list = P.mlist; oa.xw = P.xw; oa.tn = tn; oa.sched = sched; oa.gg = P.gg; oa.og = want_aplanes ? P.tw.og : nullptr;
            oa.gxw_acc = nsteps > 0 ? P.gxw : nullptr;
            if (launch_og(f, oa, 48, nsteps > 0, N, st)) return 1;
            if (fork2) { HIPCK(hipEventRecord(forks->fork[0], st)); HIPCK(hipStreamWaitEvent(forks->s, forks->fork[0], 0)); }
            if (want_aplanes) {
                if (launch_tile_scatter(f, P.tw, P.counters + 1, P.mlist, P.xw, tn, *grads, 48, N, s_atail, sched, presort)) return 1;
            }
        }
    } else if (want_aplanes) {
        ScatterArgs sa; memset(&sa, 0, sizeof(sa));
        sa.f = *f; sa.count = P.counters + 1; sa.list = P.mlist; sa.xw = P.xw; sa.tn = tn; sa.sched = sched; sa.gg = P.gg; sa.g = det_mode() ? gdet : *grads; sa.plane_mask = 63;
        hipStream_t ss = st;
        if (side) { HIPCK(hipEventRecord(sides->fork[0], st)); HIPCK(hipStreamWaitEvent(sides->s, sides->fork[0], 0)); ss = sides->s; forked = true; }
        ProfScope ps(PK_APP_SCATTER, ss);
        if (det_mode() ? launch_scatter_det(sa, 48, N, ss) : launch_scatter(f, sa, 48, N, tn, ss)) return 1;
    }
    LAUNCHCK();
    // render-MLP weight gradients
    // (round 5: at a non-keyframe time on one stream their ring / reduce jobs ride in the velocity net's two launches at the end of the call)
    WgradJobs mlp_wj; mlp_wj.n = 0; ReduceJobs mlp_rj; mlp_rj.n = 0;
    const bool merge_wgrad = fl && nsteps > 0 && !fork2;
    {
        WgradJobs& wj = mlp_wj; ReduceJobs& rj = mlp_rj;
        const size_t fs = APP_F_ROWS * REGF, bs = APP_B_ROWS * REGF;
        auto add = [&](const float* A, int a_regs, const float* B, int b_regs, float* slabs, float* gW, float* gb, int out, int in, int sk) {
            WgradJob& J = wj.j[wj.n++];
            memset(&J, 0, sizeof(J));
            J.A = A; J.a_tile_stride = bs; J.a_regs = a_regs; J.B = B; J.B2 = nullptr; J.b_tile_stride = fs; J.b_regs = b_regs;
            J.bmode = BM_RAW; J.count = P.counters + 1; J.cap_tiles = (int)P.cap_tiles; J.nrep = 1; J.a_rep_stride = 0; J.b_rep_stride = 0;
            J.slabs = slabs; J.nslab = NSLAB;
            ReduceJob& Q = rj.j[rj.n++];
            memset(&Q, 0, sizeof(Q));
            Q.slabs = slabs; Q.nslab = NSLAB; Q.MTA = a_regs / 16; Q.KTB = b_regs / 16; Q.gW = gW; Q.gb = gb; Q.out = out; Q.in = in;
            Q.row_kind = RK_NATURAL; Q.slot_kind = sk; Q.scale = 1.f;
        };
        float* sl = P.slabs;
        if (grads->rW[2] || grads->rb[2]) add(P.app_b + 0, 16, P.app_f + 160 * REGF, 64, sl + 0 * (size_t)NSLAB_MAX * SLAB_FLOATS, grads->rW[2], grads->rb[2], 3, 128, SK_HIDDEN);
        if (grads->rW[1] || grads->rb[1]) add(P.app_b + 16 * REGF, 64, P.app_f + 96 * REGF, 64, sl + 1 * (size_t)NSLAB_MAX * SLAB_FLOATS, grads->rW[1], grads->rb[1], 128, 128, SK_HIDDEN);
        if (grads->rW[0] || grads->rb[0]) add(P.app_b + 80 * REGF, 64, P.app_f + 32 * REGF, 64, sl + 2 * (size_t)NSLAB_MAX * SLAB_FLOATS, grads->rW[0], grads->rb[0], 128, 110, SK_RENDER_IN);
        if (grads->basis) add(P.app_b + 144 * REGF, 16, P.app_f + 0, 32, sl + 3 * (size_t)NSLAB_MAX * SLAB_FLOATS, grads->basis, nullptr, f->app_dim, f->Ca, SK_HIDDEN);
        if (!merge_wgrad && launch_wgrad(wj, rj, s_atail)) return 1;
    }
    // composites + raw2alpha
    WeightArgs wa; memset(&wa, 0, sizeof(wa));
    wa.R = R; wa.S = S; wa.xpre = P.xpre; wa.xw = P.xw; wa.distance_scale = f->distance_scale; wa.weight_thres = f->weight_thres;
    wa.far_ = f->far_; wa.mflag = P.mflag; wa.off_m = P.off_m; wa.rgbs = P.rgbs; wa.rgb_pre = P.rgb_pre;
    wa.g_rgb = g_rgb; wa.g_depth = g_depth; wa.g_acc = g_acc; wa.g_weight = g_weights; wa.gxpre = P.gxpre;
    wa.white_bg = (flags & NVFI_WHITE_BG) ? 1 : 0;
    if (launch_weights_bwd(wa, sd)) return 1;
    // density planes + coordinate grads
    DensityArgs da; memset(&da, 0, sizeof(da));
    da.f = *f; da.count = P.counters + 0; da.list = P.vlist; da.xw = P.xw; da.xpre = P.xpre; da.tn = tn; da.sched = sched;
    da.gxpre = P.gxpre; memset(&da.g, 0, sizeof(da.g)); da.mflag = P.mflag; da.gxw = P.gxw; da.gxk = nsteps > 0 ? P.gxk : nullptr;
    const bool want_dplanes = grads->dps[0] || grads->dpt[0];
    if (P.tiles) {
        // one pass over the samples: per-plane value gradients (og) for the tile scatter and, at non-keyframe times, the coordinate gradients
        if (nsteps > 0 || want_dplanes) {
            ProfScope ps(PK_DENSITY_BWD, sd);
            OgArgs oa; memset(&oa, 0, sizeof(oa));
            oa.f = *f; oa.count = P.counters + 0; oa.list = P.vlist; oa.xw = P.xw; oa.tn = tn; oa.sched = sched; oa.gxpre = P.gxpre; oa.og = want_dplanes ? twd.og : nullptr;
            oa.mflag = P.mflag; oa.gxw = P.gxw; oa.gxk = nsteps > 0 ? P.gxk : nullptr;
            if (launch_og(f, oa, 24, nsteps > 0, N, sd)) return 1;
        }
        if (fork2) { HIPCK(hipEventRecord(forks->fork[1], st)); HIPCK(hipStreamWaitEvent(forks->s, forks->fork[1], 0)); }
        if (want_dplanes) {
            ProfScope ps(PK_DENSITY_SCATTER, s_dtail);
            if (launch_tile_scatter(f, twd, P.counters + 0, P.vlist, P.xw, tn, *grads, 24, N, s_dtail, sched, presort)) return 1;
        }
        if (fork) { HIPCK(hipEventRecord(forks->join, forks->s)); HIPCK(hipStreamWaitEvent(st, forks->join, 0)); }
    } else if (nsteps > 0) { ProfScope ps(PK_DENSITY_BWD, st); if (launch_density_bwd(da, N, st)) return 1; }
    if (!P.tiles && want_dplanes) {
        ScatterArgs sa; memset(&sa, 0, sizeof(sa));
        sa.f = *f; sa.count = P.counters + 0; sa.list = P.vlist; sa.xw = P.xw; sa.tn = tn; sa.sched = sched; sa.gxpre = P.gxpre; sa.g = det_mode() ? gdet : *grads; sa.plane_mask = 63;
        hipStream_t ss = st;
        if (side) { HIPCK(hipEventRecord(sides->fork[1], st)); HIPCK(hipStreamWaitEvent(sides->s, sides->fork[1], 0)); ss = sides->s; forked = true; }
        ProfScope ps(PK_DENSITY_SCATTER, ss);
        if (det_mode() ? launch_scatter_det(sa, 24, N, ss) : launch_scatter(f, sa, 24, N, tn, ss)) return 1;
    }
    if (det_mode() && launch_det_finish(f, P.shadow, grads, st)) return 1;
    // RK2 adjoint + velocity-net weight gradients
    if (nsteps > 0) {
        Rk2Args ra;
        warp_uni_args(f, VI, P.counters + 3, P.rlist, P.xw, N, WarpSchedule{nsteps, dts, tcs, sched, nullptr, nullptr},
                      WarpStash{P.zst, P.x0st, P.rec, P.gst, P.cap_tiles, warp_stash_x4(f) ? 1 : 0 /* what the forward wrote */}, P.gxk, &ra);
        // NVFI_RK2_FUSE (default 1): vel_fuse.hip - the adjoint AND the four 128 x 128 weight gradients in one persistent kernel (no g_1..g_4
        // stash, no second pass over the z stash); 0: k_rk2_split_bwd + k_wgrad_ring8 over the full adjoint stash (warp_uni_bwd)
        float* vslabs = (fork2 || merge_wgrad) ? P.slabs2 : P.slabs;      // (merged launches: the render MLP's slabs in P.slabs are still live)
        int fused_nslab = 0;
        if (fuse) {
            FuseBwdArgs fa; memset(&fa, 0, sizeof(fa));
            fa.r = ra; fa.slabs = vslabs; fa.layer_stride = (int64_t)NSLAB * SLAB_FLOATS; fa.slab_floats = SLAB_FLOATS;
            for (int l = 0; l < 6; ++l) fa.t4[l] = VI.t4[l];
            fa.imgT = VI.x6t;
            if (launch_rk2_fuse_bwd(fa, N, NSLAB, &fused_nslab, st)) return 1;
        } else if (warp_uni_bwd(VI, ra, nullptr, st)) return 1;
        if (launch_vel_wgrad(P.zst, P.x0st, P.gst, P.counters + 3, (int)P.cap_tiles, 2 * nsteps, BM_SILU, vslabs, NSLAB,
                             grads->vW, grads->vb, 1.f, st, fused_nslab, merge_wgrad ? &mlp_wj : nullptr, merge_wgrad ? &mlp_rj : nullptr)) return 1;
    }
    if (fork2) { HIPCK(hipEventRecord(forks->join, forks->s)); HIPCK(hipStreamWaitEvent(st, forks->join, 0)); }
    if (forked) { HIPCK(hipEventRecord(sides->join, sides->s)); HIPCK(hipStreamWaitEvent(st, sides->join, 0)); }
    return 0;
}

// velocity-net weight gradients from the (z, x0, g) stashes of nrep evaluations
// fused_nslab > 0: the slabs of the four hidden layers were already written (fused_nslab of them each) by k_rk2_fuse_bwd - only the two
// edge layers are contracted here, the reduce covers all six
int launch_vel_wgrad(const float* zst, const float* x0st, const float* gst, const int* count, int cap_tiles, int nrep,
                     int act_mode, float* slabs, int nslab, float* const* gW, float* const* gb, float scale, hipStream_t st, int fused_nslab,
                     const WgradJobs* pre_w, const ReduceJobs* pre_r) {
    WgradJobs wj; wj.n = 0; ReduceJobs rj; rj.n = 0;
    if (pre_w) wj = *pre_w;          // jobs of the same call that share the two launches (the render MLP's, render.hip)
    if (pre_r) rj = *pre_r;
    const size_t zs = VEL_Z_REGS * REGF, gs = VEL_G_REGS * REGF, xs = VEL_X0_REGS * REGF;
    for (int l = 0; l < 6; ++l) {
        if (!gW[l] && !gb[l]) continue;
        if (fused_nslab > 0 && l >= 1 && l <= 4) {
            ReduceJob& Q = rj.j[rj.n++];
            memset(&Q, 0, sizeof(Q));
            Q.slabs = slabs + (size_t)l * nslab * SLAB_FLOATS; Q.nslab = fused_nslab; Q.MTA = 4; Q.KTB = 4; Q.gW = gW[l]; Q.gb = gb[l];
            Q.out = 128; Q.in = 128; Q.row_kind = RK_NATURAL; Q.slot_kind = SK_HIDDEN; Q.scale = scale;
            continue;
        }
        WgradJob& J = wj.j[wj.n++];
        memset(&J, 0, sizeof(J));
        J.A = gst + (size_t)l * 64 * REGF; J.a_tile_stride = gs; J.a_regs = l < 5 ? 64 : 16; J.a_rep_stride = (size_t)cap_tiles * gs;
        if (l == 0) { J.B = x0st; J.b_tile_stride = xs; J.b_regs = 16; J.bmode = BM_RAW; J.b_rep_stride = (size_t)cap_tiles * xs; }
        else { J.B = zst + (size_t)(l - 1) * 64 * REGF; J.b_tile_stride = zs; J.b_regs = 64; J.bmode = act_mode; J.b_rep_stride = (size_t)cap_tiles * zs; }
        J.B2 = nullptr; J.count = count; J.cap_tiles = cap_tiles; J.nrep = nrep;
        J.slabs = slabs + (size_t)l * nslab * SLAB_FLOATS; J.nslab = nslab;
        ReduceJob& Q = rj.j[rj.n++];
        memset(&Q, 0, sizeof(Q));
        Q.slabs = J.slabs; Q.nslab = nslab; Q.MTA = J.a_regs / 16; Q.KTB = J.b_regs / 16; Q.gW = gW[l]; Q.gb = gb[l];
        Q.out = l < 5 ? 128 : 6; Q.in = l == 0 ? 28 : 128; Q.row_kind = RK_NATURAL; Q.slot_kind = l == 0 ? SK_VEL_IN : SK_HIDDEN; Q.scale = scale;
    }
    return launch_wgrad(wj, rj, st);
}

