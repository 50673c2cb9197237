// advect.hip - the adjoint of integrate_pos for a call whose two times are host scalars (nvfi_advect_grad, include/nvfi_hip.h): the gradient of a
// loss on the advected points with respect to the STARTING positions and to weight_net, every gate / rejection decision held fixed.
// Reference semantics: autograd through models/tensorf_keyframe.py:575-611 (integrate_pos) around models/velocity_field.py:21-98.
//
// Nothing is kept between the forward (nvfi_integrate_pos, which saves no stash) and this call: the warp is run again here on the uniform
// schedule from t to t_target in training form, and the render's own adjoint chain follows on that stash:
//   k_advect_pack                                  (N,3) x / g_xk -> dense float4, the identity list, the device count
//   warp_uni_fwd (warp.h)                          the stash-writing warp of a training render (advect_kind(f); plain stash, z_x4 = 0)
//   warp_uni_bwd(gx0)                              k_rk2_split_bwd<true>: the unfused adjoint, which also stores the gradient at the start
//   launch_vel_wgrad(fused_nslab = 0)              six ring jobs + the slab reduce, ACCUMULATED into grads->vW / vb
// The adjoint is always the unfused pair, whatever NVFI_RK2_FUSE says: the fused kernel (vel_fuse.hip) has no position output.
// Everything behind the pack kernel is advect_chain (advect.h), the host-side entry nvfi_flow_loss_bwd (flowloss.hip) and nvfi_advect_grad_pt
// (advect_pt.hip: per-point times, the same chain on a device-side schedule table) share.  Which launcher runs, and how its argument block is
// filled, is warp.hip's: the chain names the schedule and the rooms.
// All on the caller's stream, no host synchronisation.
#include <string.h>
#include "common.h"
#include "pde.h"
#include "render.h"
#include "x6.h"
#include "advect.h"

#define ADV_NSLAB 256                            // slab capacity of a weight-gradient job (one per CU), as the render's
#define ADV_SLAB_FLOATS (128 * 128 + 128)        // (launch_vel_wgrad strides the six jobs by nslab slabs of this size)

// thread i: point i of both dense images and of the identity list; thread 0 also writes the count the uniform kernels read from device memory
__global__ __launch_bounds__(256) void k_advect_pack(int64_t N, const float* __restrict__ x, const float* __restrict__ g, float4* __restrict__ xw,
                                                     float4* __restrict__ gxk, int* __restrict__ list, int* __restrict__ count) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0) *count = (int)N;
    if (i >= N) return;
    xw[i] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.f);
    gxk[i] = make_float4(g[3 * i], g[3 * i + 1], g[3 * i + 2], 0.f);
    list[i] = (int)i;
}
// no step: the gradient passes through unchanged
__global__ __launch_bounds__(256) void k_advect_copy(int64_t n, const float* __restrict__ src, float* __restrict__ dst) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// sized like plan_render's `nsteps > 0 && train` block: whole 128-point workgroups of stash tiles, two evaluations per step, the records
void plan_advect(const nvfi_field_desc* f, int64_t N, int nsteps, WarpKind kind, void* ws, AdvectPlan* P) {
    Bump B{(char*)ws, 0, 0};
    const unsigned own = f->frags ? 0 : warp_need(kind, WARP_ADJOINT);   // without a fragment cache the images are packed into the call's own room
    P->cap_tiles = (N + WG_SAMPLES - 1) / WG_SAMPLES * 4;
    P->count = B.take<int>(16);
    P->list = B.take<int>(N);
    P->xw = B.take<float4>(N + 1);
    P->gxk = B.take<float4>(N);
    P->vel_frag = (own & VI_VEL) ? B.take<float>(VEL_FRAG_FLOATS) : nullptr;
    P->vel_x4 = (own & VI_X4F) ? B.take<float>(VEL_X4F_FLOATS) : nullptr;
    P->vel_x4b = (own & VI_X4B) ? B.take<float>(VEL_X4B_FLOATS) : nullptr;
    P->x6img = (own & VI_X6) ? (void*)B.take<float>(X6_IMAGE_BYTES / 4) : nullptr;
    P->slabs = B.take<float>((int64_t)ADV_NSLAB * ADV_SLAB_FLOATS * 6);
    const int64_t nev = 2 * (int64_t)nsteps;
    P->zst = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_Z_REGS * REGF));
    P->x0st = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_X0_REGS * REGF));
    P->gst = B.take<float>(nev * P->cap_tiles * (int64_t)(VEL_G_REGS * REGF));
    P->rec = B.take<float>((int64_t)nsteps * RK_NF * N);
    P->total = align_up(B.off, 256);
}

static int advect_check(const nvfi_field_desc* f, int64_t N, float t, float t_target, float* dts, float* tcs, int* nsteps) {
    if (N < 0) return nvfi_fail(2, "nvfi_advect_grad: N=%lld", (long long)N);
    if (int rc = check_vel_call("nvfi_advect_grad", f, N, VEL_CALL_NO_FP16IN)) return rc;
    *nsteps = rk_schedule_to(*f, t, t_target, dts, tcs);
    if (*nsteps < 0) return nvfi_fail(2, "t=%g -> t_target=%g needs more than %d RK2 steps", t, t_target, MAX_RK_STEPS);
    return 0;
}

extern "C" int nvfi_advect_grad_workspace_bytes(const nvfi_field_desc* f, int64_t N, float t, float t_target, int64_t* bytes) {
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    int nsteps;
    if (int rc = advect_check(f, N, t, t_target, dts, tcs, &nsteps)) return rc;
    AdvectPlan P; plan_advect(f, N, nsteps, advect_kind(f), nullptr, &P);
    *bytes = (N == 0 || nsteps == 0) ? 256 : P.total;
    return 0;
}

extern "C" int nvfi_advect_grad(const nvfi_field_desc* f, int64_t N, const float* x, float t, float t_target, const float* g_xk, float* g_x,
                                const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    int nsteps;
    if (int rc = advect_check(f, N, t, t_target, dts, tcs, &nsteps)) return rc;
    if (N == 0) return 0;
    if (!g_xk) return nvfi_fail(2, "nvfi_advect_grad: g_xk is NULL");
    if (nsteps == 0) {
        if (g_x) { hipLaunchKernelGGL(k_advect_copy, dim3((unsigned)((3 * N + 255) / 256)), dim3(256), 0, st, 3 * N, g_xk, g_x); LAUNCHCK(); }
        return 0;
    }
    if (!x || !grads) return nvfi_fail(2, "nvfi_advect_grad: x and grads must be non-NULL");
    const WarpKind kind = advect_kind(f);
    AdvectPlan P; plan_advect(f, N, nsteps, kind, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld bytes, got %lld", (long long)P.total, (long long)workspace_bytes);
    hipLaunchKernelGGL(k_advect_pack, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, x, g_xk, P.xw, P.gxk, P.list, P.count);
    LAUNCHCK();
    return advect_chain(f, P, N, WarpSchedule{nsteps, dts, tcs, nullptr, nullptr, nullptr}, kind, g_x, grads, st);
}

// the launches behind the caller's pack kernel (advect.h): shared with nvfi_flow_loss_bwd (flowloss.hip) and nvfi_advect_grad_pt (advect_pt.hip)
int advect_chain(const nvfi_field_desc* f, const AdvectPlan& P, int64_t N, const WarpSchedule& s, WarpKind kind, float* g_x,
                 const nvfi_grads* grads, hipStream_t st) {
    VelImages VI;
    if (int rc = vel_images(f, warp_need(kind, WARP_ADJOINT), VelImageRoom{P.vel_frag, nullptr, P.vel_x4, P.vel_x4b, nullptr, P.x6img, nullptr}, &VI, nullptr, 0, st)) return rc;
    Rk2Args ra;
    warp_uni_args(f, VI, P.count, P.list, P.xw, N, s, WarpStash{P.zst, P.x0st, P.rec, P.gst, P.cap_tiles, 0}, P.gxk, &ra);
    if (warp_uni_fwd(f, kind, VI, nullptr, ra, true, st)) return 1;
    if (warp_uni_bwd(VI, ra, g_x, st)) return 1;
    return launch_vel_wgrad(P.zst, P.x0st, P.gst, P.count, (int)P.cap_tiles, 2 * s.nsteps, BM_SILU, P.slabs, ADV_NSLAB, grads->vW, grads->vb, 1.f, st, 0);
}
