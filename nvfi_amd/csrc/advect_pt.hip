// advect_pt.hip - the adjoint of integrate_pos for PER-POINT times (nvfi_advect_pt_steps / nvfi_advect_grad_pt, include/nvfi_hip_advect_pt.h): the chain of
// advect.hip (advect_chain, advect.h) with the two numbers of a step - dt and its start time - read per point from a schedule table instead of
// from the argument block.
//   k_advect_pt_steps       steps[i] = rk_steps(dt_max, t_i, t_target_i) and the histogram of the step counts (the host plans its chunks from it)
//   k_advect_pt_sched       pack (as k_advect_pack) + the table dt[s][i], tcur[s][i] for s < max_steps.  A point that has finished at step s has
//                           dt = 0 there (a dead step: the per-point-times kernels leave it where it is, record flag 4, and the adjoint treats the
//                           step as the identity); its tcur is the time it rests at, so the stash rows of a dead step come from an ordinary,
//                           finite evaluation.  A point whose schedule does not fit in max_steps (or in MAX_RK_STEPS) takes NO step in this call
//                           - every step dead, its gradient passes through - and is counted in info[0]: never truncated.
//   advect_chain(pt table)  warp_uni_fwd / warp_uni_bwd (warp.h) on a WarpSchedule that names the table: k_rk2_x6_uni_pt / k_rk2_split_uni<true, true>,
//                           k_rk2_split_bwd<., true>; launch_vel_wgrad over 2 max_steps evaluations
// rk_steps (common.h) stays the one copy of the step loop: both kernels call it.  All on the caller's stream, no host synchronisation.
#include <string.h>
#include "common.h"
#include "advect.h"

#define ADV_PT_BINS (MAX_RK_STEPS + 2)          // step counts 0 .. 64, then the points beyond

__global__ __launch_bounds__(256) void k_advect_pt_steps(float dtm, int64_t N, const float* __restrict__ t, const float* __restrict__ tg,
                                                         int32_t* __restrict__ steps, unsigned long long* __restrict__ hist) {
    __shared__ int h[ADV_PT_BINS];
    for (int k = threadIdx.x; k < ADV_PT_BINS; k += blockDim.x) h[k] = 0;
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < N) {
        float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
        const int n = rk_steps(dtm, t[i], tg[i], dts, tcs);
        if (steps) steps[i] = n;
        atomicAdd(&h[n < 0 ? MAX_RK_STEPS + 1 : n], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ADV_PT_BINS; k += blockDim.x)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
}

// thread i: point i of both dense images, of the identity list and of the schedule table; thread 0 also writes the device count
__global__ __launch_bounds__(256) void k_advect_pt_sched(float dtm, int64_t N, int max_steps, const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ t, const float* __restrict__ tg, float4* __restrict__ xw,
                                                         float4* __restrict__ gxk, int* __restrict__ list, int* __restrict__ count,
                                                         float* __restrict__ tdt, float* __restrict__ ttc, unsigned long long* __restrict__ info) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0) *count = (int)N;
    if (i >= N) return;
    xw[i] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.f);
    gxk[i] = make_float4(g[3 * i], g[3 * i + 1], g[3 * i + 2], 0.f);
    list[i] = (int)i;
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    const float ti = t[i];
    int n = rk_steps(dtm, ti, tg[i], dts, tcs);
    if (n < 0 || n > max_steps) {                // left out of this call, and counted
        n = 0;
        if (info) atomicAdd(info, 1ull);
    }
    const float rest = n > 0 ? tcs[n - 1] - dts[n - 1] : ti;
    for (int s = 0; s < max_steps; ++s) {
        tdt[(size_t)s * N + i] = s < n ? dts[s] : 0.f;
        ttc[(size_t)s * N + i] = s < n ? tcs[s] : rest;
    }
}

// what: 0 for the step count (every mode has an integrator), VEL_CALL_NO_FP16IN for the adjoint
static int advect_pt_check(const char* who, const nvfi_field_desc* f, int64_t N, unsigned what) {
    if (N < 0) return nvfi_fail(2, "%s: N=%lld", who, (long long)N);
    return check_vel_call(who, f, N, what);
}
static int advect_pt_check_grad(const char* who, const nvfi_field_desc* f, int64_t N, int max_steps) {
    if (int rc = advect_pt_check(who, f, N, VEL_CALL_NO_FP16IN)) return rc;
    if (max_steps < 0 || max_steps > MAX_RK_STEPS) return nvfi_fail(2, "%s: max_steps=%d is outside 0 .. %d", who, max_steps, MAX_RK_STEPS);
    return 0;
}
// the rooms of advect_chain for max_steps steps, the schedule table behind them
static int64_t advect_pt_plan(const nvfi_field_desc* f, int64_t N, int max_steps, WarpKind kind, void* ws, AdvectPlan* P, float** table) {
    plan_advect(f, N, max_steps, kind, ws, P);
    *table = ws ? reinterpret_cast<float*>((char*)ws + P->total) : nullptr;
    return P->total + align_up(2 * (int64_t)max_steps * N * (int64_t)sizeof(float), 256);
}

extern "C" int nvfi_advect_pt_steps(const nvfi_field_desc* f, int64_t N, const float* t, const float* t_target, int32_t* steps, int64_t* hist66,
                                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = advect_pt_check("nvfi_advect_pt_steps", f, N, 0)) return rc;
    if (!hist66) return nvfi_fail(2, "nvfi_advect_pt_steps: hist66 is NULL");
    if (N > 0 && (!t || !t_target)) return nvfi_fail(2, "nvfi_advect_pt_steps: t and t_target must be non-NULL");
    HIPCK(hipMemsetAsync(hist66, 0, ADV_PT_BINS * sizeof(int64_t), st));
    if (N == 0) return 0;
    hipLaunchKernelGGL(k_advect_pt_steps, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dt_max_of(*f), N, t, t_target, steps,
                       reinterpret_cast<unsigned long long*>(hist66));
    LAUNCHCK();
    return 0;
}

extern "C" int nvfi_advect_grad_pt_workspace_bytes(const nvfi_field_desc* f, int64_t N, int max_steps, int64_t* bytes) {
    if (int rc = advect_pt_check_grad("nvfi_advect_grad_pt", f, N, max_steps)) return rc;
    AdvectPlan P; float* table;
    const int64_t total = advect_pt_plan(f, N, max_steps, advect_kind(f), nullptr, &P, &table);
    *bytes = (N == 0 || max_steps == 0) ? 256 : total;
    return 0;
}

extern "C" int nvfi_advect_grad_pt(const nvfi_field_desc* f, int64_t N, const float* x, const float* t, const float* t_target, int max_steps,
                                   const float* g_xk, float* g_x, const nvfi_grads* grads, int64_t* info, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = advect_pt_check_grad("nvfi_advect_grad_pt", f, N, max_steps)) return rc;
    if (N == 0) return 0;
    if (!g_xk) return nvfi_fail(2, "nvfi_advect_grad_pt: g_xk is NULL");
    if (max_steps == 0) {
        if (g_x) HIPCK(hipMemcpyAsync(g_x, g_xk, 3 * N * sizeof(float), hipMemcpyDeviceToDevice, st));      // no step: the gradient passes through
        return 0;
    }
    if (!x || !t || !t_target || !grads) return nvfi_fail(2, "nvfi_advect_grad_pt: x, t, t_target and grads must be non-NULL");
    const WarpKind kind = advect_kind(f);
    AdvectPlan P; float* table;
    const int64_t total = advect_pt_plan(f, N, max_steps, kind, workspace, &P, &table);
    if (!workspace || total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld bytes, got %lld", (long long)total, (long long)workspace_bytes);
    if (info) HIPCK(hipMemsetAsync(info, 0, sizeof(int64_t), st));
    float* tdt = table; float* ttc = table + (int64_t)max_steps * N;
    hipLaunchKernelGGL(k_advect_pt_sched, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dt_max_of(*f), N, max_steps, x, g_xk, t, t_target, P.xw,
                       P.gxk, P.list, P.count, tdt, ttc, reinterpret_cast<unsigned long long*>(info));
    LAUNCHCK();
    return advect_chain(f, P, N, WarpSchedule{max_steps, nullptr, nullptr, nullptr, tdt, ttc}, kind, g_x, grads, st);
}
