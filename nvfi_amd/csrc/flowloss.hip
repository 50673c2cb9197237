// flowloss.hip - optical-flow supervision of a TRAINING render (nvfi_flow_loss_fwd / nvfi_flow_loss_bwd, include/nvfi_hip.h; the reference has no
// such term): the flow map of the render's own appearance-masked samples, its loss against a target flow, and all gradients - the weights' for
// the render backward (g_weights), the velocity net's through the adjoint of integrate_pos.
//
// nvfi_flow_loss_fwd runs behind nvfi_render_fwd* (NVFI_TRAIN) and in front of its backward.  It reads the render workspace READ-ONLY (mlist,
// off_m, the device counts, xw.w); everything it writes lives in the call's own workspace:
//   k_fl_gather       x_j = normalize_coord(o_r + d_r z_j), z_j = the depth the render used (jitter and the t_min rule are in it), one thread per
//                     masked entry, sized from the device count; + the per-point times of the integrator and the masked count for the backward
//   warp_points       Phi(x_j) = integrate_pos(x_j, t, t + dt), the no-grad per-point integrator of nvfi_integrate_pos / nvfi_render_flow (warp.h), in place
//   k_fl_ray          one wave per ray, lanes as in k_flow_final: flow2d[r] as an ordered sum, the error against the target, the ray's loss term (fp64)
//   k_fl_mean         ONE workgroup: the valid count n and the mean in a fixed order (reduce.h's ordered workgroup sum)
//   k_fl_grad         one thread per masked entry: g_weights (written behind a zero fill, or added to) and g_xd, the gradient at the displaced point
// nvfi_flow_loss_bwd handles the entries [first, first + chunk_cap) of the masked list, clipped on the device:
//   k_fl_pack         the chunk's dense positions, g_xd, the identity list, the device count
//   advect_chain      the chain of nvfi_advect_grad (advect.h): stash-writing uniform warp, unfused adjoint, weight-gradient jobs
// No MFMA code is instantiated here, no host synchronisation, no float atomics of its own: two calls repeat bit for bit.
#include <string.h>
#include "reduce.h"
#include "render.h"
#include "x6.h"
#include "advect.h"

#define FL_MEAN_THREADS 1024
#define FL_HDR_INTS 16                 // [0] masked count (clipped to the capacity), [1] n, the number of valid rays

struct FlowLossPlan {
    int* hdr; double* lterm; float2* err; int* vflag;
    float4 *xt, *xd, *gxd; float* tb;
    float* vel_frag; void* x6img;
    int64_t persist;                   // bytes in front of the backward's chunk plan
    int64_t total;
};

struct FlArgs {
    nvfi_field_desc f;
    int64_t R; int64_t cap;
    const int* count; const int* off_m; const int* list; const float4* xw;
    const float* o; const float* d; const float* weight;
    float t, t1;
    float4* xt; float4* xd; float4* gxd; float* tb;
    int* hdr; double* lterm; float2* err; int* vflag;
    const float* pose; float focal;
    const float* target; const uint8_t* valid; int kind; float delta;
    float grad_scale; const float* grad_scale_dev; int add_gw;
    float* loss; float* flow2d; float* g_weights;
};

static void plan_flow_loss(const nvfi_field_desc* f, int64_t R, int nsteps, int64_t chunk_cap, void* ws, FlowLossPlan* P, AdvectPlan* A) {
    Bump B{(char*)ws, 0, 0};
    const int64_t cap = R * (int64_t)f->n_samples;
    const unsigned own = f->frags ? 0 : warp_need(warp_kind(f, false, true), WARP_POINTS);      // the forward's integrator; the chunk plan has its own
    P->hdr = B.take<int>(FL_HDR_INTS);
    P->lterm = B.take<double>(R);
    P->err = B.take<float2>(R);
    P->vflag = B.take<int>(R);
    P->xt = B.take<float4>(cap); P->xd = B.take<float4>(cap); P->gxd = B.take<float4>(cap);
    P->tb = B.take<float>(2 * cap);
    P->vel_frag = (own & VI_VEL) ? B.take<float>(VEL_FRAG_FLOATS) : nullptr;
    P->x6img = (own & VI_X6) ? (void*)B.take<float>(X6_IMAGE_BYTES / 4) : nullptr;
    P->persist = align_up(B.off, 256);
    P->total = P->persist;
    if (nsteps > 0 && chunk_cap > 0) {
        plan_advect(f, chunk_cap, nsteps, advect_kind(f), ws ? (char*)ws + P->persist : nullptr, A);
        P->total += A->total;
    }
}

// pi(P'_j) - pi(P_j) of masked entry i, (0, 0) behind the guard; c1: the camera coordinates of the displaced point.  pi is flow.hip's flow_project -
// c = R^T (P - o_cam), u = focal c_x / d, v = -(focal c_y / d), d = -c_z - but the DIFFERENCE of the two projections is formed from the
// displacement in camera coordinates, dc = R^T (P' - P):  u' - u = focal (dc_x d - c_x dd) / (d d'),  dd = d' - d.  Two pixel positions of several
// hundred whose difference is a few pixels would lose in the subtraction the digits this form keeps; P' == P gives exact zeros.
// The ONE copy: k_fl_ray and k_fl_grad see the same bits.  ps: the 12 pose floats, which every thread loads ONCE into registers (fl_pose), as
// k_flow_final does, not once per entry
__device__ __forceinline__ void fl_pose(const FlArgs& a, float* ps) {
#pragma unroll
    for (int k = 0; k < 12; ++k) ps[k] = a.pose[k];
}
__device__ __forceinline__ bool fl_delta(const FlArgs& a, const float* ps, int64_t i, float& du, float& dv, float* c1) {
    const nvfi_field_desc& f = a.f;
    const float4 x0 = a.xt[i], x1 = a.xd[i];
    const float q0[3] = {x0.x, x0.y, x0.z}, q1[3] = {x1.x, x1.y, x1.z};
    float p[3], dp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float hk = (f.aabb[3 + k] - f.aabb[k]) / 2.f;
        p[k] = f.aabb[k] + (q0[k] + 1.f) * hk - ps[4 * k + 3];
        dp[k] = (q1[k] - q0[k]) * hk;
    }
    float c0[3], dc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        c0[m] = ps[m] * p[0] + ps[4 + m] * p[1] + ps[8 + m] * p[2];
        dc[m] = ps[m] * dp[0] + ps[4 + m] * dp[1] + ps[8 + m] * dp[2];
        c1[m] = c0[m] + dc[m];
    }
    const float d0 = -c0[2], d1 = -c1[2], dd = -dc[2];
    const bool keep = !(d1 < 1e-3f);
    const float den = d0 * d1;
    du = keep ? a.focal * (dc[0] * d0 - c0[0] * dd) / den : 0.f;
    dv = keep ? -(a.focal * (dc[1] * d0 - c0[1] * dd) / den) : 0.f;
    return keep;
}

// one thread per masked entry: dense index n = ray * S + sample -> the position the render gave the sample before its warp moved it
__global__ __launch_bounds__(256) void k_fl_gather(FlArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t M = (int64_t)*a.count < a.cap ? (int64_t)*a.count : a.cap;
    if (i == 0) a.hdr[0] = (int)M;
    if (i >= M) return;
    const nvfi_field_desc& f = a.f;
    const int n = a.list[i];
    const int64_t r = n / f.n_samples;
    const float z = a.xw[n].w;
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xn[c] = norm_coord(f, c, a.o[3 * r + c] + a.d[3 * r + c] * z);
    a.xt[i] = make_float4(xn[0], xn[1], xn[2], a.t);
    a.xd[i] = make_float4(xn[0], xn[1], xn[2], 0.f);
    a.tb[i] = a.t; a.tb[a.cap + i] = a.t1;
}

__device__ __forceinline__ float fl_rho(int kind, float delta, float e) {
    if (kind == 0) return e * e;
    const float ae = fabsf(e);
    return ae <= delta ? 0.5f * e * e : delta * (ae - 0.5f * delta);
}
__device__ __forceinline__ float fl_drho(int kind, float delta, float e) {
    if (kind == 0) return 2.f * e;
    return fabsf(e) <= delta ? e : (e > 0.f ? delta : -delta);
}

// one wave per ray; lane = (entry slot e of 8, component c of 8) as in k_flow_final, of which c = 6, 7 (u, v) work: eight entries per pass, every
// lane sums its own entries in list order, then the eight slots are added in a fixed tree - the same bits every call
__global__ __launch_bounds__(256) void k_fl_ray(FlArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;                              // (whole waves leave: the shuffles below see full waves)
    const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
    const int c = lane & 7, e0 = lane >> 3;
    float s = 0.f;
    if (c >= 6) {
        float ps[12];
        fl_pose(a, ps);
        for (int i = b0 + e0; i < b1; i += 8) {
            const float w = a.weight[a.list[i]];
            float du, dv, c1[3];
            fl_delta(a, ps, i, du, dv, c1);
            s += w * (c == 6 ? du : dv);
        }
    }
    s += __shfl_xor(s, 8); s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
    const float sv = __shfl(s, 7);
    if ((lane == 6 || lane == 7) && a.flow2d) a.flow2d[2 * r + lane - 6] = s;
    if (lane == 6) {
        const float tu = a.target[2 * r], tv = a.target[2 * r + 1];
        const bool ok = (!a.valid || a.valid[r] != 0) && isfinite(tu) && isfinite(tv);
        const float eu = s - tu, ev = sv - tv;
        a.err[r] = ok ? make_float2(eu, ev) : make_float2(0.f, 0.f);
        a.vflag[r] = ok ? 1 : 0;
        a.lterm[r] = ok ? (double)fl_rho(a.kind, a.delta, eu) + (double)fl_rho(a.kind, a.delta, ev) : 0.0;
    }
}

// n = number of valid rays, loss = sum of the per-ray terms / (2 n): every thread sums its stride, then the workgroup's ordered sums (reduce.h)
__global__ __launch_bounds__(FL_MEAN_THREADS) void k_fl_mean(FlArgs a) {
    __shared__ double part[FL_MEAN_THREADS / 64];
    __shared__ int npart[FL_MEAN_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int64_t i = tid; i < a.R; i += FL_MEAN_THREADS) { s += a.lterm[i]; n += a.vflag[i]; }
    block_sum_ordered<FL_MEAN_THREADS / 64, 1>(&s, part, tid & 63, tid >> 6);
    block_sum_ordered<FL_MEAN_THREADS / 64, 1>(&n, npart, tid & 63, tid >> 6);
    if (tid == 0) {
        a.hdr[1] = n;
        if (a.loss) { a.loss[0] = n > 0 ? (float)(s / (2.0 * (double)n)) : 0.f; a.loss[1] = (float)n; }
    }
}

// one thread per masked entry: the weight's gradient and the gradient at the displaced point, every discrete decision held fixed
__global__ __launch_bounds__(256) void k_fl_grad(FlArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.hdr[0]) return;
    const nvfi_field_desc& f = a.f;
    const int n = a.list[i];
    const int64_t r = n / f.n_samples;
    const int nv = a.hdr[1];
    const bool ok = a.vflag[r] != 0 && nv > 0;
    float gu = 0.f, gv = 0.f;
    if (ok) {
        const double k = (double)a.grad_scale * (a.grad_scale_dev ? (double)a.grad_scale_dev[0] : 1.0) / (2.0 * (double)nv);
        const float2 e = a.err[r];
        gu = (float)(k * (double)fl_drho(a.kind, a.delta, e.x)); gv = (float)(k * (double)fl_drho(a.kind, a.delta, e.y));
    }
    float du, dv, c1[3], ps[12];
    fl_pose(a, ps);
    const bool keep = fl_delta(a, ps, i, du, dv, c1);
    if (a.g_weights) {
        const float g = ok ? gu * du + gv * dv : 0.f;
        if (a.add_gw) a.g_weights[n] += g; else a.g_weights[n] = g;
    }
    float4 gx = zero4();
    if (ok && keep) {
        const float w = a.weight[n];
        const float dd = -c1[2];
        // J^T g_r with du/dc = focal (1/d, 0, c_x/d^2), dv/dc = -focal (0, 1/d, c_y/d^2)
        const float gc[3] = {a.focal * gu / dd, -(a.focal * gv / dd), a.focal * (gu * c1[0] - gv * c1[1]) / (dd * dd)};
        float g3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float hk = (f.aabb[3 + k] - f.aabb[k]) / 2.f;
            g3[k] = w * hk * (ps[4 * k] * gc[0] + ps[4 * k + 1] * gc[1] + ps[4 * k + 2] * gc[2]);
        }
        gx = make_float4(g3[0], g3[1], g3[2], 0.f);
    }
    a.gxd[i] = gx;
}

// thread i: entry first + i of the masked list as point i of the chunk's dense images and identity list; thread 0 also writes the chunk's count
__global__ __launch_bounds__(256) void k_fl_pack(int64_t first, int64_t cap, const int* __restrict__ hdr, const float4* __restrict__ xt,
                                                 const float4* __restrict__ gxd, float4* __restrict__ xw, float4* __restrict__ gxk,
                                                 int* __restrict__ list, int* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t left = (int64_t)hdr[0] - first;
    const int64_t cnt = left <= 0 ? 0 : (left > cap ? cap : left);
    if (i == 0) *count = (int)cnt;
    if (i >= cnt) return;
    const float4 x = xt[first + i];
    xw[i] = make_float4(x.x, x.y, x.z, 0.f);
    gxk[i] = gxd[first + i];
    list[i] = (int)i;
}

static int flow_loss_check(const char* who, const nvfi_field_desc* f, int64_t R, float t, float dt, float* dts, float* tcs, int* nsteps) {
    if (R <= 0) return nvfi_fail(2, "%s: R=%lld, at least one ray is needed", who, (long long)R);
    if (int rc = check_vel_call(who, f, 0, VEL_CALL_NO_FP16IN)) return rc;
    if (f->n_samples < 1 || R * (int64_t)f->n_samples >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "%s: R * n_samples = %lld is more than one call holds", who, (long long)(R * (int64_t)f->n_samples));
    *nsteps = rk_schedule_to(*f, t, t + dt, dts, tcs);
    if (*nsteps < 0) return nvfi_fail(2, "%s: dt=%g needs more than %d RK2 steps", who, dt, MAX_RK_STEPS);
    return 0;
}
static int flow_loss_ws_check(const char* who, const FlowLossPlan& P, const void* ws, int64_t ws_bytes) {
    if (!ws || ws_bytes < P.total) return nvfi_fail(4, "%s: workspace of %lld bytes, %lld needed", who, (long long)(ws ? ws_bytes : 0), (long long)P.total);
    if ((uintptr_t)ws & 15) return nvfi_fail(4, "%s: the workspace must be 16-byte aligned", who);
    return 0;
}

extern "C" int nvfi_flow_loss_workspace_bytes(const nvfi_field_desc* f, int64_t R, float t, float dt, int64_t chunk_cap, int64_t* bytes) {
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    int nsteps;
    if (!f || !bytes) return nvfi_fail(2, "nvfi_flow_loss_workspace_bytes: f and bytes must not be NULL");
    if (int rc = flow_loss_check("nvfi_flow_loss_workspace_bytes", f, R, t, dt, dts, tcs, &nsteps)) return rc;
    if (chunk_cap < 1) return nvfi_fail(2, "nvfi_flow_loss_workspace_bytes: chunk_cap=%lld", (long long)chunk_cap);
    FlowLossPlan P; AdvectPlan A;
    plan_flow_loss(f, R, nsteps, chunk_cap, nullptr, &P, &A);
    *bytes = P.total;
    return 0;
}

extern "C" int nvfi_flow_loss_fwd(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t, float dt, int flags,
                                  const float* weights, const float* pose3x4, int H, int W, float focal,
                                  const float* target, const uint8_t* valid, int kind, float huber_delta,
                                  float grad_scale, const float* grad_scale_dev, int loss_flags,
                                  float* loss, float* flow2d, float* g_weights,
                                  const void* render_workspace, int64_t render_workspace_bytes, int64_t chunk_cap,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    (void)H; (void)W;                                  // (the principal point cancels in a difference of two projections)
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    int nsteps;
    if (!f) return nvfi_fail(2, "nvfi_flow_loss_fwd: f must not be NULL");
    if (!(flags & NVFI_TRAIN)) return nvfi_fail(2, "nvfi_flow_loss_fwd supervises a TRAINING render: flags without NVFI_TRAIN (nvfi_render_flow is the inference branch)");
    if (int rc = flow_loss_check("nvfi_flow_loss_fwd", f, R, t, dt, dts, tcs, &nsteps)) return rc;
    if (!pose3x4) return nvfi_fail(2, "nvfi_flow_loss_fwd: pose3x4 is NULL");
    if (!target) return nvfi_fail(2, "nvfi_flow_loss_fwd: target is NULL");
    if (kind != 0 && kind != 1) return nvfi_fail(2, "nvfi_flow_loss_fwd: kind=%d (0 l2, 1 huber)", kind);
    if (kind == 1 && !(huber_delta > 0.f)) return nvfi_fail(2, "nvfi_flow_loss_fwd: huber_delta=%g", huber_delta);
    if (loss_flags & ~NVFI_FLOWLOSS_ADD_GW) return nvfi_fail(2, "nvfi_flow_loss_fwd: unknown loss_flags %d", loss_flags);
    if (chunk_cap < 1) return nvfi_fail(2, "nvfi_flow_loss_fwd: chunk_cap=%lld", (long long)chunk_cap);
    if (!rays_o || !rays_d || !weights || !render_workspace) return nvfi_fail(2, "nvfi_flow_loss_fwd: rays, weights and the render workspace must not be NULL");
    FlowLossPlan P; AdvectPlan A;
    plan_flow_loss(f, R, nsteps, chunk_cap, workspace, &P, &A);
    if (int rc = flow_loss_ws_check("nvfi_flow_loss_fwd", P, workspace, workspace_bytes)) return rc;
    RenderPlan RP;     // the forward's, for reading: the masked list, its per-ray offsets, the device-side counts, the sample depths
    if (int rc = render_plan_at(f, R, flags, t, const_cast<void*>(render_workspace), render_workspace_bytes, &RP)) return rc;
    const int64_t N = RP.N;
    FlArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.R = R; a.cap = N; a.count = RP.counters + 1; a.off_m = RP.off_m; a.list = RP.mlist; a.xw = RP.xw;
    a.o = rays_o; a.d = rays_d; a.weight = weights; a.t = t; a.t1 = t + dt;
    a.xt = P.xt; a.xd = P.xd; a.gxd = P.gxd; a.tb = P.tb;
    a.hdr = P.hdr; a.lterm = P.lterm; a.err = P.err; a.vflag = P.vflag;
    a.pose = pose3x4; a.focal = focal;
    a.target = target; a.valid = valid; a.kind = kind; a.delta = huber_delta;
    a.grad_scale = grad_scale; a.grad_scale_dev = grad_scale_dev; a.add_gw = (loss_flags & NVFI_FLOWLOSS_ADD_GW) ? 1 : 0;
    a.loss = loss; a.flow2d = flow2d; a.g_weights = g_weights;
    const dim3 gN((unsigned)((N + 255) / 256)), b256(256);
    hipLaunchKernelGGL(k_fl_gather, gN, b256, 0, st, a);
    LAUNCHCK();
    if (nsteps > 0) {
        const WarpKind kind = warp_kind(f, false, true);
        VelImages VI;
        if (int rc = vel_images(f, warp_need(kind, WARP_POINTS), VelImageRoom{P.vel_frag, nullptr, nullptr, nullptr, nullptr, P.x6img}, &VI, nullptr, 0, st)) return rc;
        if (warp_points(f, kind, VI, nullptr, WarpPoints{a.count, N, nullptr, P.xd, nullptr, P.tb, P.tb + N, 0, MAX_RK_STEPS}, st)) return 1;
    }
    hipLaunchKernelGGL(k_fl_ray, dim3((unsigned)((R + 3) / 4)), b256, 0, st, a);
    LAUNCHCK();
    hipLaunchKernelGGL(k_fl_mean, dim3(1), dim3(FL_MEAN_THREADS), 0, st, a);
    LAUNCHCK();
    if (g_weights && !a.add_gw)
        if (int rc = launch_zero(g_weights, N * (int64_t)sizeof(float), st)) return rc;
    hipLaunchKernelGGL(k_fl_grad, gN, b256, 0, st, a);
    LAUNCHCK();
    return 0;
}

extern "C" int nvfi_flow_loss_bwd(const nvfi_field_desc* f, int64_t R, float t, float dt, int64_t first, int64_t chunk_cap,
                                  const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    int nsteps;
    if (!f) return nvfi_fail(2, "nvfi_flow_loss_bwd: f must not be NULL");
    if (int rc = flow_loss_check("nvfi_flow_loss_bwd", f, R, t, dt, dts, tcs, &nsteps)) return rc;
    const int64_t cap = R * (int64_t)f->n_samples;
    if (chunk_cap < 1 || first < 0 || first >= cap) return nvfi_fail(2, "nvfi_flow_loss_bwd: first=%lld, chunk_cap=%lld outside the %lld entries of the call", (long long)first, (long long)chunk_cap, (long long)cap);
    if (nsteps > 0 && !grads) return nvfi_fail(2, "nvfi_flow_loss_bwd: grads is NULL");
    FlowLossPlan P; AdvectPlan A;
    plan_flow_loss(f, R, nsteps, chunk_cap, workspace, &P, &A);
    if (int rc = flow_loss_ws_check("nvfi_flow_loss_bwd", P, workspace, workspace_bytes)) return rc;
    if (nsteps == 0) return 0;                         // Phi is the identity: nothing reaches the net
    hipLaunchKernelGGL(k_fl_pack, dim3((unsigned)((chunk_cap + 255) / 256)), dim3(256), 0, st, first, chunk_cap, P.hdr, P.xt, P.gxd, A.xw, A.gxk, A.list, A.count);
    LAUNCHCK();
    return advect_chain(f, A, chunk_cap, WarpSchedule{nsteps, dts, tcs, nullptr, nullptr, nullptr}, advect_kind(f), nullptr, grads, st);
}
