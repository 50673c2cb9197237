/* nvfi_hip_advect_pt.h - an addition to ABI v5 of libnvfi_hip.so: differentiable advection with per-point times (csrc/advect_pt.hip).
 * Included by nvfi_hip.h behind nvfi_advect_grad, inside its extern "C" block; not meant to be included alone (it needs nvfi_field_desc and
 * nvfi_grads).  Binding: nvfi_amd/_lib.py: ADDITIONS, one row per prototype below, in this order. */
#ifndef NVFI_HIP_H
#error "include nvfi_hip.h, which includes this file"
#endif
#ifndef NVFI_HIP_ADVECT_PT_H
#define NVFI_HIP_ADVECT_PT_H
/* ---- the adjoint of nvfi_advect_grad (nvfi_hip.h), every rule of it
 *      kept, for xk_i = integrate_pos(x_i, t_i, t_target_i) with t, t_target (N) DEVICE arrays.  The times get no gradient.  The forward is
 *      nvfi_integrate_pos; the backward runs the warp again with every point on its own schedule (a table in the workspace, built on the device
 *      from the step loop nvfi_integrate_pos takes): a point with fewer than max_steps steps rests for the remaining ones - its position stays,
 *      the step is the identity in the adjoint and adds exactly nothing to the net's gradient.  The cost of a call is N x max_steps, whatever the
 *      points need: sort the points by step count and give every chunk its own max_steps (TensorVMKeyframeTimeKplane.advect_pt does).
 *      nvfi_advect_pt_steps: steps[i] (may be NULL) = the RK2 steps of point i, -1 beyond 64; hist66[0..64] = points per step count, hist66[65] =
 *        points beyond 64 (WRITTEN, cleared first; 66 int64 in device memory).  What a host needs to plan: no host synchronisation here.
 *      nvfi_advect_grad_pt: g_x (N,3), WRITTEN (may be NULL); grads->vW / vb ACCUMULATED.  A point whose schedule does not fit in max_steps is NOT
 *        truncated: it takes no step in this call, g_x_i = g_xk_i, it adds nothing to the net's gradient, and info[0] (device, may be NULL; WRITTEN)
 *        counts such points.  max_steps == 0 or N == 0: g_x = g_xk, nothing else runs.  The workspace is nvfi_advect_grad's at max_steps steps plus
 *        the table (8 bytes per point and step).  All launches go to `stream`; no host synchronisation.
 *      Errors, before any launch: (2) N < 0 or N >= 2^31 - 256, use_vel == 0, vel_fp16 modes 1 / 2, max_steps outside 0 .. 64, a NULL array;
 *      (4) workspace under nvfi_advect_grad_pt_workspace_bytes(f, N, max_steps). */
int nvfi_advect_pt_steps(const nvfi_field_desc* f, int64_t N, const float* t, const float* t_target, int32_t* steps, int64_t* hist66, void* stream);
int nvfi_advect_grad_pt_workspace_bytes(const nvfi_field_desc* f, int64_t N, int max_steps, int64_t* bytes);
int nvfi_advect_grad_pt(const nvfi_field_desc* f, int64_t N, const float* x, const float* t, const float* t_target, int max_steps,
                        const float* g_xk /* (N,3) */, float* g_x /* (N,3) or NULL, WRITTEN */,
                        const nvfi_grads* grads /* vW / vb ACCUMULATED, the rest ignored */, int64_t* info /* device, [0] = points left out, or NULL */,
                        void* workspace, int64_t workspace_bytes, void* stream);
#endif
