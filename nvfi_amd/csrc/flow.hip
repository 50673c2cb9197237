// flow.hip - velocity, scene-flow and optical-flow maps of an eval-mode render (nvfi_render_flow; the reference has no counterpart: the fifth
// output of its Renderer is called `velocity` but is the mask map).
//
// An inference-only branch of the render built like the mask branch (render_blocks.hip: nvfi_render_mask): it runs behind nvfi_render_fwd on the
// workspace that call filled and walks the appearance-masked list (mlist, off_m, counters) without the masked count ever reaching the host.
//   k_flow_gather    x_j (the UN-warped normalised sample position, the fp32 arithmetic of k_sample_fill) and t for every masked sample,
//                    into the compacted arrays xt (the velocity net's input) and xd (the integrator's in-place state), + the per-point times
//   launch_vel_eval  v_g(x_j, t): the gated VelBasis evaluation behind nvfi_vel_eval, sized by the device-side count
//   warp_points      Phi(x_j) = integrate_pos(x_j, t, t + dt): the per-point integrator behind nvfi_integrate_pos (warp.h: x6; vel_fp16 bit 3 or
//                    NVFI_INTEGRATE_X6=0: the fp32 MFMA kernel), in place on xd, sized by the device-side count
//   k_flow_final     per-ray ordered sums through off_m with the world scaling and the pinhole projection in the epilogue
// No MFMA code is instantiated here (the launchers live in vel.hip / vel_x6.hip / vel_x6w.hip), so the unit needs no packed-fp32 fence.
#include <string.h>
#include "common.h"
#include "render.h"
#include "warp.h"

struct FlowArgs {
    nvfi_field_desc f;
    int64_t R; int64_t cap;
    const int* count; const int* inside; const int* off_m; const int* list;
    const float* o; const float* d; const float* weight;
    float t, t1;
    float4* xt; float4* xd; const float4* vg; float* tb;
    const float* pose; int H, W; float focal;
    float* vel_map; float* flow_map; float* flow2d;
};

// one thread per masked sample: dense index n = ray * S + sample -> the position k_sample_fill gave it before the warp moved it
__global__ __launch_bounds__(256) void k_flow_gather(FlowArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= *a.count || i >= a.cap) return;
    const nvfi_field_desc& f = a.f;
    const int n = a.list[i];
    const int S = f.n_samples;
    const int64_t r = n / S;
    const int j = n - (int)(r * S);
    const float o[3] = {a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
    const float d[3] = {a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
    const float tmin = ray_tmin(f, *a.inside != 0, o, d);
    const float rng = (float)j + 0.f;           // (eval: no jitter)
    const float step = f.step_size * rng;
    const float z = tmin + step;
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xn[c] = norm_coord(f, c, o[c] + d[c] * z);
    a.xt[i] = make_float4(xn[0], xn[1], xn[2], a.t);
    a.xd[i] = make_float4(xn[0], xn[1], xn[2], 0.f);
    a.tb[i] = a.t; a.tb[a.cap + i] = a.t1;
}

// pixel offset (u - W/2, v - H/2) of world point P: c = R^T (P - o_cam), u = W/2 + focal c_x / (-c_z), v = H/2 - focal c_y / (-c_z); depth = -c_z
__device__ __forceinline__ void flow_project(const float* pose, float focal, const float* P, float& du, float& dv, float& depth) {
    const float q[3] = {P[0] - pose[3], P[1] - pose[7], P[2] - pose[11]};
    const float cx = pose[0] * q[0] + pose[4] * q[1] + pose[8] * q[2];
    const float cy = pose[1] * q[0] + pose[5] * q[1] + pose[9] * q[2];
    const float cz = pose[2] * q[0] + pose[6] * q[1] + pose[10] * q[2];
    depth = -cz;
    du = focal * cx / depth; dv = -(focal * cy / depth);
}

// one wave per ray; lane = (entry slot e of 8, component c of 8): c 0..2 vel_map, 3..5 flow_map, 6..7 flow2d.  A ray's list is tens of entries:
// eight entries per pass, every lane sums its own entries in list order, then the eight slots are added in a fixed tree - the same bits every call
__global__ __launch_bounds__(256) void k_flow_final(FlowArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const nvfi_field_desc& f = a.f;
    const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
    const int c = lane & 7, e0 = lane >> 3;
    const int ax = c < 3 ? c : (c < 6 ? c - 3 : 0);
    const float half = (f.aabb[3 + ax] - f.aabb[ax]) / 2.f;
    float pose[12];
    if (a.pose) {
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = a.pose[k];
    }
    float s = 0.f;
    for (int i = b0 + e0; i < b1; i += 8) {
        const float w = a.weight[a.list[i]];
        const float4 x0 = a.xt[i], x1 = a.xd[i];
        float val;
        if (c < 3) {
            const float4 v = a.vg[i];
            val = half * (c == 0 ? v.x : (c == 1 ? v.y : v.z));
        } else if (c < 6) {
            val = half * (c == 3 ? x1.x - x0.x : (c == 4 ? x1.y - x0.y : x1.z - x0.z));
        } else if (a.pose) {
            float P0[3], P1[3];
            const float q0[3] = {x0.x, x0.y, x0.z}, q1[3] = {x1.x, x1.y, x1.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float hk = (f.aabb[3 + k] - f.aabb[k]) / 2.f;
                P0[k] = f.aabb[k] + (q0[k] + 1.f) * hk; P1[k] = f.aabb[k] + (q1[k] + 1.f) * hk;
            }
            float u0, v0, z0, u1, v1, z1;
            flow_project(pose, a.focal, P0, u0, v0, z0);
            flow_project(pose, a.focal, P1, u1, v1, z1);
            val = z1 < 1e-3f ? 0.f : (c == 6 ? u1 - u0 : v1 - v0);
        } else val = 0.f;
        s += w * val;
    }
    s += __shfl_xor(s, 8); s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
    if (lane < 3) { if (a.vel_map) a.vel_map[3 * r + lane] = s; }
    else if (lane < 6) { if (a.flow_map) a.flow_map[3 * r + lane - 3] = s; }
    else if (lane < 8) { if (a.flow2d && a.pose) a.flow2d[2 * r + lane - 6] = s; }
}

extern "C" int nvfi_render_flow(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t, float dt, int flags,
                                const float* weights, const float* pose3x4, int H, int W, float focal, float* vel_map, float* flow_map,
                                float* flow2d, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (R <= 0) return 0;
    if (flags & NVFI_TRAIN) return nvfi_fail(2, "nvfi_render_flow is an inference branch: NVFI_TRAIN renders have none");
    if (check_vel_call("nvfi_render_flow", f, 0, VEL_CALL_NO_FP16IN)) return 2;       // (the descriptor and R * S: render_plan_at and the forward)
    if (!(flags & NVFI_WANT_FLOW)) return nvfi_fail(2, "nvfi_render_flow needs a workspace planned with NVFI_WANT_FLOW in flags");
    RenderPlan P;     // the forward's: the masked list, its per-ray offsets, the device-side counts, and the flow branch's own room
    const int rc = render_plan_at(f, R, flags, t, workspace, workspace_bytes, &P);
    if (rc == 4)
        return nvfi_fail(2, "workspace of %lld bytes, a plan with NVFI_WANT_FLOW needs %lld: nvfi_render_flow needs a workspace planned with the flag", (long long)workspace_bytes, (long long)P.total);
    if (rc) return rc;
    const int* const count_m = P.counters + 1;
    if (!P.flow_xt) return nvfi_fail(2, "nvfi_render_flow needs a workspace planned with NVFI_WANT_FLOW in flags");
    const bool want2d = flow2d && pose3x4, want_flow = flow_map || want2d;
    if (!vel_map && !want_flow) return 0;
    // the integrator's own recurrence on the host (rk_steps): a dt that needs more steps than the library's limit is refused, not truncated
    const float t1 = t + dt;
    float dts[MAX_RK_STEPS], tcs[MAX_RK_STEPS];
    if (rk_schedule_to(*f, t, t1, dts, tcs) < 0) return nvfi_fail(2, "dt=%g needs more than %d RK2 steps", dt, MAX_RK_STEPS);
    const int64_t N = P.N;
    FlowArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.R = R; a.cap = N; a.count = count_m; a.inside = P.counters + 2; a.off_m = P.off_m; a.list = P.mlist;
    a.o = rays_o; a.d = rays_d; a.weight = weights; a.t = t; a.t1 = t1;
    a.xt = P.flow_xt; a.xd = P.flow_xd; a.vg = P.flow_vg; a.tb = P.flow_tb;
    a.pose = pose3x4; a.H = H; a.W = W; a.focal = focal;
    a.vel_map = vel_map; a.flow_map = flow_map; a.flow2d = flow2d;
    hipLaunchKernelGGL(k_flow_gather, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a);
    LAUNCHCK();
    // (vf is 0 or 3 here: WARP_X6 or WARP_FP32)
    const WarpKind kind = warp_kind(f, false, true);
    const bool warp = want_flow && t1 != t;
    const unsigned need = (vel_map ? VI_VEL : 0) | (warp ? warp_need(kind, WARP_POINTS) : 0);
    VelImages VI;
    if (int rc2 = vel_images(f, need, VelImageRoom{P.vel_frag, nullptr, nullptr, nullptr, nullptr, P.flow_x6}, &VI, nullptr, 0, st)) return rc2;
    if (vel_map) {
        VelEvalArgs va; memset(&va, 0, sizeof(va));
        va.f = *f; va.Wv = VI.VW; va.N = N; va.count = count_m; va.xt = reinterpret_cast<const float*>(P.flow_xt);
        va.u6 = reinterpret_cast<float*>(P.flow_vg); va.u_stride = 4; va.gated = 1;
        if (launch_vel_eval(va, st)) return 1;
    }
    if (warp && warp_points(f, kind, VI, nullptr, WarpPoints{count_m, N, nullptr, P.flow_xd, nullptr, P.flow_tb, P.flow_tb + N, 0, MAX_RK_STEPS}, st)) return 1;
    hipLaunchKernelGGL(k_flow_final, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, a);
    LAUNCHCK();
    return 0;
}
