// render.h - the render step's internal header: argument blocks of its kernels, the workspace plan, and the launchers of its units -
// render_rays.hip (per-ray stages), render_app.hip (appearance MLP), render.hip (plan, forward, backward), render_blocks.hip (stand-alone
// calls and the inference mask branch); the plane-gradient scatters are scatter.h's
#pragma once
#include <string.h>
#include "common.h"
#include "vel.h"
#include "scatter.h"

struct SampleArgs {
    nvfi_field_desc f;
    int64_t R;
    const float* o; const float* d; const float* u;
    int train;
    const int* inside;
    float4* xw; float* xpre; uint8_t* valid; int* cnt;
    uint8_t* rflag; int* cnt_r;   // valid AND inside the velocity gate: the samples the RK2 warp has to touch (NULL: not wanted)
    // k_sample_fill (sampling + both ordered compact lists in one launch): look-back status words (zero at launch), the lists, their totals
    unsigned long long* lb; int* vlist; int* rlist; int* total_v; int* total_r;
};

struct DensityArgs {
    nvfi_field_desc f;
    const int* count; int64_t n_direct;
    const int* list;
    const float4* xw;
    float tn; int per_point_t;
    const float* sched;       // optional device-side schedule record (common.h); NULL: the by-value tn
    float* xpre; float* feat_out; float* sigma_out;
    // backward
    const float* gxpre;
    nvfi_grads g;
    const uint8_t* mflag; const float4* gxw; float4* gxk;
};

struct WeightArgs {
    int64_t R; int S;
    const float* xpre; const float4* xw;
    float distance_scale, weight_thres, far_;
    float* weight; uint8_t* mflag; float* acc; float* depth; int* cnt_m;
    const float* sel;   // nvfi_render_fwd_select: s(x) per dense sample index, written for the valid samples (objects.hip: k_select_fwd); NULL otherwise
    // k_weights_fill (weights + the ordered list of appearance-masked samples in one launch)
    unsigned long long* lb; int* off_m_out; int* mlist; int* total_m;
    // backward
    const int* off_m; const float4* rgbs; const float4* rgb_pre;
    const float* g_rgb; const float* g_depth; const float* g_acc; const float* g_weight;
    float* gxpre;
    int white_bg;
};

struct FinalArgs {
    int64_t R;
    const int* off_m; const int* mlist;
    const float* weight; const float4* rgbs; const float* acc;
    int white_bg;
    float4* rgb_pre; float* rgb;
    // the call's counters (k_counters' job) written by workgroup 0 of the same launch; NULL: not wanted
    const int* c; int nsteps; int64_t* counters_out; const float* sched;
    // nvfi_render_fwd_mse: F.mse_loss(rgb, target) and its gradient from the same launch (target == NULL: not wanted).  g_rgb_out[i] =
    // loss_scale * 2 (rgb[i] - target[i]) / (3 R); per-workgroup partial sums, summed in workgroup order by the last one to finish (ticket)
    const float* target; float* g_rgb_out; float* loss_out; float* partial; int* ticket; float loss_scale;
};

struct AppArgs {
    nvfi_field_desc f;
    RenderFrags W;
    const int* count; int64_t n_direct;
    const int* list;
    const float4* xw;
    float tn; int per_point_t; int S;
    const float* sched;
    const float* rays_d; const float* view_per_point;
    float4* rgbs; int rgb_dense;
    const float* feat48;   // (M,48) plane-product features of the masked samples by compact index (k_app_feat): no plane gather in k_app_fwd
    const float* feat_in;  // (N, app_dim) appearance features given by the caller (renderModule as a stand-alone call): no plane gather, no basis_mat
    float* stash_f; float* stash_b;
    unsigned* relu_mask;   // [tile][layer 1 | layer 2][lo | hi][64 lanes]: bit s of a lane = (hidden activation register s > 0), written by k_app_fwd<stash>,
                           // read by k_app_bwd instead of the 128 activation rows themselves (1 KB instead of 32 KB per tile)
    // backward
    nvfi_grads g;
    const float* g_rgb; const float4* rgb_pre; const float* weight;
    float4* gxw;
    float* gg;           // (M,48) per-sample channel gradients for k_plane_scatter (NULL: scatter in-kernel)
    int plane_tail;      // 1: coordinate gradients of the plane lookups (+ in-kernel scatter when gg is NULL) are computed here; 0: k_og does it (or nobody needs them)
};

// device-side schedule (k_sched / k_prologue): the field, the device time (NULL: the host's t holds) and the host's plan to fall back to
struct SchedArgs {
    nvfi_field_desc f; const float* t_dev; int flags; int nsteps_plan; float tn_plan; float dt_plan[4]; float tc_plan[4]; float* sched;
};

// the workspace of a render call.  nvfi_render_fwd fills it; the backward and the inference branches behind the forward (mask, flow,
// objects, export) plan the same call again and read it
struct RenderPlan {
    int64_t N, cap_tiles;
    int nsteps;
    float* sched;       // device-side schedule record (SCHED_FLOATS), written by k_sched when the call passes a device time
    int* counters;      // [0] V, [1] M, [2] inside flag
    int *cnt_v, *off_v, *cnt_m, *off_m, *vlist, *mlist, *cnt_r, *off_r, *rlist;
    uint8_t *valid, *mflag, *rflag;
    float4 *xw, *rgbs, *rgb_pre, *gxw, *gxk;
    float *xpre, *gxpre;
    float *vel_frag, *render_frag, *vel_x4, *vel_x4b; void* img16; void* x6img; void* x6imgT;
    TileWork tw2; float* slabs2;
    float *app_f, *app_b, *zst, *x0st, *rec, *gst, *gg, *maskv, *mask_frag;
    float4 *flow_xt, *flow_xd, *flow_vg; float *flow_tb, *flow_x6;   // NVFI_WANT_FLOW: the flow branch's room (flow.hip)
    float *sel, *sel_frag;     // NVFI_WANT_SELECT: s(x) per dense sample index and the MaskField fragments of nvfi_render_fwd_select (objects.hip)
    unsigned* app_relu;
    float *slabs;
    long long* shadow;         // NVFI_DETERMINISTIC: int64 fixed-point images of the 12 plane gradients
    int64_t zero_bytes;        // counters .. end of the sort histograms / look-back words: zeroed by the forward's single fill (or k_prologue)
    unsigned long long *lb_s, *lb_w;   // look-back status words of k_sample_fill / k_weights_fill
    float* mse_part;
    TileWork tw; bool tiles;   // sorted-tile plane scatter (scatter.hip); tiles = false: grid too large, atomic scatter instead
    int64_t total;
};
// THE way to a RenderPlan: descriptor check, RK2 schedule of t (refused beyond MAX_RK_STEPS), plan, and - unless ws is NULL, the
// *_workspace_bytes calls - the size check (code 4; P->total is set).  base / dts / tcs: the schedule for callers that want it, or NULL
int check_desc(const nvfi_field_desc* f);
int render_plan_at(const nvfi_field_desc* f, int64_t R, int flags, float t, void* ws, int64_t ws_bytes, RenderPlan* P, float* base = nullptr,
                   float* dts = nullptr, float* tcs = nullptr);
// s(x) = sum_k select_k softmax(MaskField(x))_k at the warped keyframe positions of the valid samples, into sel[dense sample index] (objects.hip);
// frag: room for the packed MaskField fragments (64 K floats), N: the launch capacity, count_v: the device-side valid count
int launch_select(const nvfi_mask_desc* m, const float* select, const int* count_v, const int* vlist, const float4* xw, float* sel, float* frag,
                  int64_t N, hipStream_t st);

#ifdef __HIPCC__
// first sample depth of a ray (tensorf_base.py:294-300); k_sample / k_sample_fill and the flow branch's position rebuild share it
__device__ __forceinline__ float ray_tmin(const nvfi_field_desc& f, bool inside, const float* o, const float* d) {
    if (inside) return f.near_;
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float vec = d[c] == 0.f ? 1e-6f : d[c];
        float ra = (f.aabb[3 + c] - o[c]) / vec;
        float rb = (f.aabb[c] - o[c]) / vec;
        m = fmaxf(m, fminf(ra, rb));
    }
    return fminf(fmaxf(m, f.near_), f.far_);
}
#endif

// render_rays.hip
int launch_ray_head(const SchedArgs& sc, int64_t R, const float* rays_o, int* zero_from, int64_t zero_bytes, int* inside, bool fused, hipStream_t st);
int launch_sample(const SampleArgs& sa, int* off_v, int* off_r, bool fused, hipStream_t st);
int launch_weights_fwd(const WeightArgs& wa, bool fused, hipStream_t st);
int launch_final_fwd(FinalArgs fa, int64_t* counters, bool fused, hipStream_t st);
int launch_weights_bwd(const WeightArgs& wa, hipStream_t st);
int launch_density_bwd(const DensityArgs& da, int64_t N, hipStream_t st);
// render_app.hip
int launch_app_fwd(const AppArgs& aa, int64_t cap_samples, bool stash, hipStream_t st);
int launch_app_bwd(const AppArgs& aa, int64_t cap_samples, hipStream_t st);
// render.hip
int launch_vel_wgrad(const float* zst, const float* x0st, const float* gst, const int* count, int cap_tiles, int nrep,
                     int act_mode, float* slabs, int nslab, float* const* gW, float* const* gb, float scale, hipStream_t st, int fused_nslab = 0,
                     const WgradJobs* pre_w = nullptr, const ReduceJobs* pre_r = nullptr);
