/*
 * nvfi_hip.h - C ABI of the MI355X-native NVFi hot path (libnvfi_hip.so, hand-written HIP for gfx950).
 *
 * The reference has no FFI layer: its hot path is Python calling ATen ops.  This ABI is what the
 * host-side mirror (nvfi_amd/models) binds through ctypes; each entry point names the reference
 * interface it replaces.  Plain pointers and sizes only: every pointer below is a DEVICE pointer
 * unless stated, `stream` is a hipStream_t passed as void*, the caller owns every buffer, nothing
 * is allocated inside (workspace sizes are queried first).  All calls are asynchronous on
 * `stream` - none of them waits for the device - with the documented exceptions that hand a value back to the host or are diagnostics:
 * nvfi_pde_loss_ex / nvfi_pde_loss_split when `host_info` is non-NULL, nvfi_prof_collect, nvfi_selftest, and nvfi_prof_enable(1) (it drops a
 * marker launch on the null stream and waits for it).
 * Return value: 0 = ok, otherwise an error code; nvfi_last_error() gives the text.
 *
 * Layouts: factor planes are CHANNEL-LAST, [H][W][C] fp32 (the physical layout of a torch
 * (1,C,H,W) tensor in torch.channels_last); Linear weights are (out,in) row-major as in torch.
 */
#ifndef NVFI_HIP_H
#define NVFI_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVFI_ABI_VERSION 5

/* Field description: TensorVMKeyframeTimeKplane state that reaches the hot path
 * (reference models/tensorf_keyframe.py:37-134, models/tensorf_base.py:133-227). */
typedef struct nvfi_field_desc {
    int32_t G[3];            /* gridSize x,y,z */
    int32_t K;               /* num_keyframes */
    int32_t Cd, Ca, app_dim; /* 24, 48, 32 in every shipped config */
    int32_t n_samples;       /* nSamples (tensorf_base.py:223) */
    int32_t use_vel;         /* cfg.use_vel */
    int32_t gate_sur;        /* 0 VelocityAABB(eps), 1 VelocityAABBSur (velocity_field.py:21-51) */
    int32_t has_amask;       /* alphaMask present (used in eval only, tensorf_keyframe.py:656) */
    int32_t shading;         /* shadingMode (tensorf_base.py:184-197): 0 MLP_PE (app_dim 32 + MLPRender_PE), 1 SH (app_dim 27, SHRender: no MLP) */
    int32_t vel_fp16;        /* ABI v4, opt-in (0 = off, the default and the parity mode; 2 = as 1 but with fp32 products emulated by TWO binary16
                              * terms per operand, three MFMAs, ~2^-21 relative per product): 1 = every NO-GRAD back-advection (nvfi_integrate_pos,
                              * the warp of eval-mode renders, nvfi_compute_alpha) evaluates VelBasis with fp16-input MFMAs (weights and layer
                              * inputs rounded to binary16, fp32 accumulation) - the counterpart of the reference's autocast switch
                              * --disable_fp32 (train_nvfi.py:96,144) for inference; training renders, the PDE term and all gradients stay fp32.
                              * Bit 2 (+4, round 4, opt-in): the velocity warp of TRAINING renders runs its FORWARD on the one-term fp16-input MFMA too
                              * (pre-activations stashed in fp32; the adjoint and the weight gradients stay fp32 MFMA on those stashes - the
                              * arithmetic of a forward under autocast with an fp32 backward; the PDE term and the render MLP stay fp32).
                              * 3 = x6 (round 5): fp32 products of the hidden layers formed EXACTLY from three bfloat16 terms per operand on the 16-bit
                              * matrix pipe - same results as the fp32 MFMA kernels to rounding order, and since round 6 what 0 selects for every
                              * no-grad back-advection as well (eval renders and the PDE prefilter since round 5; nvfi_integrate_pos and
                              * nvfi_compute_alpha now).  Bit 3 (+8): keep the fp32 MFMA kernels for those two calls (A/B reference). */
    int32_t am_dims[3];      /* alpha volume W,H,D */
    float aabb[6];           /* min xyz, max xyz */
    float near_, far_, step_size;
    float density_shift, distance_scale, weight_thres, alpha_thres, tmax;
    float gate_lo[3], gate_hi[3]; /* velocity gate box in normalised coordinates */
    const float* dps[3];     /* density_plane_space[i]  [G_b][G_a][Cd] */
    const float* dpt[3];     /* density_plane_time[i]   [K][G_c][Cd]   */
    const float* aps[3];     /* app_plane_space[i]      [G_b][G_a][Ca] */
    const float* apt[3];     /* app_plane_time[i]       [K][G_c][Ca]   */
    const float* basis;      /* basis_mat.weight (app_dim, Ca) */
    const float* rW[3];      /* renderModule.mlp.{0,2,4}.weight */
    const float* rb[3];
    const float* vW[6];      /* vel_net.weight_net Linear weights (6 layers) */
    const float* vb[6];
    const float* aW[6];      /* vel_net.a_weight_net */
    const float* ab[6];
    const float* amask;      /* alpha volume (D,H,W) or NULL */
    const float* frags;      /* ABI v5: fragment cache written by nvfi_pack_frags for THESE weights, or NULL (the render / PDE calls then repack
                              * the weights into their own workspace, as in v1-v4) */
} nvfi_field_desc;

/* Gradient buffers, same shapes/layouts as the parameters; kernels ACCUMULATE (+=) into them.
 * A NULL pointer skips that gradient. */
typedef struct nvfi_grads {
    float* dps[3]; float* dpt[3]; float* aps[3]; float* apt[3];
    float* basis;
    float* rW[3]; float* rb[3];
    float* vW[6]; float* vb[6];
    float* aW[6]; float* ab[6];
} nvfi_grads;

#define NVFI_TRAIN     1  /* training mode: jitter used, alpha mask ignored, intermediates kept for backward */
#define NVFI_WHITE_BG  2  /* rgb += 1-acc  (white_bg or the random-white coin, tensorf_keyframe.py:740) */
#define NVFI_TRANSFER  4  /* transfer_vel: base time 0 (models/nvfi.py:30) */
#define NVFI_WANT_MASK 8  /* plan workspace room for nvfi_render_mask (mask_field attached) */
#define NVFI_WANT_FLOW 32 /* plan workspace room for nvfi_render_flow */
#define NVFI_WANT_SELECT 64 /* plan workspace room for nvfi_render_fwd_select (one float per sample + the packed MaskField) */
#define NVFI_BWD_FORK 16  /* nvfi_render_bwd at a keyframe time: the density half of the backward may run on a library-owned side stream beside the
                           * appearance half (joined before the call returns); for callers that drive a single stream */

/* counters written by nvfi_render_fwd (device int64[8]):
 * 0 valid samples V, 1 warped samples N, 2 appearance-masked samples M, 3 velocity-net evaluations, 7 device-time plan mismatch (nvfi_render_fwd_t) */
#define NVFI_NCOUNTERS 8

const char* nvfi_last_error(void);
int nvfi_abi_version(void);

/* ---- render: replaces NVFi.render_ray / TensorVMKeyframeTimeKplane.forward + render_pts
 *      (models/nvfi.py:27-31, models/tensorf_keyframe.py:613-755) for one chunk of R rays. */
int nvfi_render_workspace_bytes(const nvfi_field_desc* f, int64_t R, int flags, int64_t* bytes);
/* exact size for a given time t (extrapolated times need more RK2 steps, hence more stash) */
int nvfi_render_workspace_bytes_t(const nvfi_field_desc* f, int64_t R, int flags, float t, int64_t* bytes);
int nvfi_render_fwd(const nvfi_field_desc* f, int64_t R,
                    const float* rays_o, const float* rays_d, /* (R,3) */
                    const float* jitter,                     /* (R) u_r in [0,1) or NULL (eval) */
                    float t, int flags,
                    float* rgb, float* depth, float* acc,    /* (R,3) (R) (R) */
                    float* weights,                          /* (R,S) */
                    void* workspace, int64_t workspace_bytes,
                    int64_t* counters,                       /* device int64[NVFI_NCOUNTERS] or NULL */
                    void* stream);
/* backward of the call that filled `workspace` (autograd of models/tensorf_keyframe.py:613-755,
 * reference: loss.backward() at train_nvfi.py:242).  Upstream grads may be NULL (= zero). */
int nvfi_render_bwd(const nvfi_field_desc* f, int64_t R,
                    const float* rays_o, const float* rays_d, float t, int flags,
                    const float* weights,                    /* the (R,S) output of the forward */
                    const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                    const nvfi_grads* grads,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the same two calls with the frame time in DEVICE memory (ABI v3), so that a training iteration can be captured once as a hipGraph and
 *      replayed with a new time every iteration (train_nvfi.py:150-158 draws a new frame per iteration): `t` still fixes the launch plan
 *      on the host - how many RK2 steps the warp takes, hence which kernels run and how the workspace is laid out - while the kernels
 *      take the time itself from *t_dev (keyframe row, step sizes and step times are derived on the device, same arithmetic).  *t_dev
 *      must lie in the same plan class as `t` (same number of RK2 steps back to its keyframe: true for all non-keyframe frame times of
 *      the shipped configs, and for all keyframe times); if it does not, the call renders `t` and sets counters[7] = 1.
 *      t_dev == NULL / t_on_device == 0: exactly nvfi_render_fwd / nvfi_render_bwd. */
int nvfi_render_fwd_t(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, const float* jitter,
                      float t, const float* t_dev, int flags, float* rgb, float* depth, float* acc, float* weights,
                      void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream);
int nvfi_render_bwd_t(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t, int t_on_device, int flags,
                      const float* weights, const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                      const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* nvfi_render_fwd_t with the photometric loss of the training loop attached (ABI v5; train_nvfi.py:159,178: F.mse_loss(rgb_map, target)):
 * loss[0] = mean((rgb - target)^2) and g_rgb[i] = loss_scale * 2 (rgb[i] - target[i]) / (3 R) - the upstream gradient nvfi_render_bwd[_t]
 * takes - come out of the composite kernel of the same call (no nvfi_mse launch, no autograd node). */
int nvfi_render_fwd_mse(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, const float* jitter,
                        float t, const float* t_dev, int flags, float* rgb, float* depth, float* acc, float* weights,
                        void* workspace, int64_t workspace_bytes, int64_t* counters,
                        const float* target /* (R,3) */, float loss_scale, float* loss /* device float[1] */, float* g_rgb /* (R,3) */, void* stream);

/* ---- fragment cache (ABI v5).  The MFMA kernels read the nn.Linear weights of the field - renderModule.mlp + basis_mat
 *      (models/tensorf_base.py:67-98, tensorf_keyframe.py:310), vel_net.weight_net / a_weight_net (models/velocity_field.py:60-67) - in
 *      fragment order.  nvfi_pack_frags writes every fragment set the render and PDE calls use into `cache` (nvfi_frag_cache_bytes bytes,
 *      caller-owned) in ONE launch; a descriptor whose `frags` points at it makes nvfi_render_fwd[_t] / nvfi_render_bwd[_t] /
 *      nvfi_pde_loss* read it instead of repacking the weights per call (7 launches per training iteration otherwise).  The caller repacks
 *      after every change of the weights (once per optimiser step) and orders the readers behind the repack. */
int nvfi_frag_cache_bytes(const nvfi_field_desc* f, int64_t* bytes);
int nvfi_pack_frags(const nvfi_field_desc* f, void* cache, int64_t cache_bytes, void* stream);
/* id of the hipGraph capture `stream` is part of (0: not capturing; forked streams of one capture share the id).  A caller that bakes the
 * cache pointer into a captured call must have a nvfi_pack_frags node in the SAME capture (or replay the graph that holds it first): the
 * Python mirror uses this id to refuse a cache that was packed outside the capture, whatever its key says. */
int nvfi_stream_capture_id(void* stream, uint64_t* id);

/* ---- PDE regulariser: replaces NVFi.get_vel_loss (models/nvfi.py:42-84) with explicit collocation
 *      points (world space (P,3)) and raw times (P).  out (device float[4]): loss, n_kept, sum div^2,
 *      sum transport^2.  grads: vW,vb,aW,ab are accumulated scaled by `loss_scale` when non-NULL. */
/* Workspace of the PDE call, caller-allocated and physically backed whatever the kept count turns out to be: 1.6 GiB at P = 32 768,
 * 5.5 GiB at 131 072, 10.7 GiB from P = 262 144 up (the candidates are processed in chunks of 262 144; the stash of a chunk is sized for
 * every candidate kept). */
int nvfi_pde_workspace_bytes(const nvfi_field_desc* f, int64_t P, int64_t* bytes);
int nvfi_pde_loss(const nvfi_field_desc* f, int64_t P, const float* points, const float* t,
                  float loss_scale, float* out, const nvfi_grads* grads,
                  void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream);

/* same, with optional diagnostics: kept (device uint8[P]), jac (device float[n_jac][6][4], rows 3..5 zero: the loss
 * does not use the acceleration Jacobian) for the first n_jac kept points; host_info (HOST int64[2], optional): the kept count and
 * the number of prefilter net evaluations - asking for it makes the call synchronise `stream` once (the reference's
 * `if xyzt.shape[0] == 0`, nvfi.py:66, is the same wait); with host_info == NULL the call is asynchronous: the kept count never
 * leaves the device (out[1], counters[4]) and the Jacobian / adjoint passes size themselves from it. */
int nvfi_pde_loss_ex(const nvfi_field_desc* f, int64_t P, const float* points, const float* t,
                     float loss_scale, float* out, const nvfi_grads* grads,
                     void* workspace, int64_t workspace_bytes, int64_t* counters,
                     uint8_t* kept_out, float* jac_out, int64_t n_jac, int64_t* host_info, void* stream);
/* As nvfi_pde_loss_ex with the call split over two streams: out[] (the value) is complete on `stream` after the Jacobian forward; the adjoint
 * pass and the weight gradients run on `bwd_stream`, ordered behind the forward by an event.  For the reference's loop, which waits for the
 * value right after the call (train_nvfi.py:233) and then differentiates the renders: the PDE adjoint overlaps with them.  The caller
 * orders its use of `grads` and the release of `workspace` behind `bwd_stream`.  P above one chunk (262 144): one stream. */
int nvfi_pde_loss_split(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, float loss_scale,
                        float* out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters,
                        uint8_t* kept_out, float* jac_out, int64_t n_jac, int64_t* host_info, void* stream, void* bwd_stream);

/* nvfi_pde_loss with the loss scale (train_nvfi.py:229-234: vel_reg_weight, decayed every iteration) read from device memory */
int nvfi_pde_loss_dev(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, const float* loss_scale_dev,
                      float* out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream);

/* ---- mask branch of render_pts (models/tensorf_keyframe.py:673-676, 749-753) with the MaskField as train_segm.py:97-102
 *      builds it: 3 -> n_dim x n_layer (ReLU) -> mask_dim, softmax.  Call after nvfi_render_fwd with the same workspace:
 *      mask_map[R][mask_dim] = sum over appearance-masked samples of weight * softmax(MaskField(warped xyz)). Inference only
 *      (a loss on this map with all its gradients: nvfi_mask_loss_fwd / nvfi_mask_loss_bwd below). */
typedef struct nvfi_mask_desc {
    int32_t n_layer;         /* hidden layers (4) */
    int32_t n_dim;           /* hidden width (128) */
    int32_t mask_dim;        /* outputs (<= 32) */
    const float* W[5];       /* point_fc.{0..3}.weight (n_dim,3|n_dim), mask_fc.weight (mask_dim,n_dim) */
    const float* b[5];
} nvfi_mask_desc;
int nvfi_render_mask(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, float t, int flags, const float* weights,
                     float* mask_map, void* workspace, int64_t workspace_bytes, void* stream);
/* appearance-masked samples of the nvfi_render_fwd call that filled `workspace` (same f, R, t, flags): warped keyframe positions
 * xyz_out (cap,3) and dense sample indices idx_out (cap) = ray * n_samples + sample; entries beyond counters[2] are left untouched.
 * With it the host builds the train-mode (differentiable) mask branch of render_pts (models/tensorf_keyframe.py:749-753) from
 * nvfi_maskfield_fwd / nvfi_maskfield_bwd: mask_map = sum_j weight_j * MaskField(xyz_j). */
int nvfi_render_export_masked(const nvfi_field_desc* f, int64_t R, float t, int flags, void* workspace, int64_t workspace_bytes,
                              int64_t cap, float* xyz_out, int64_t* idx_out, void* stream);
/* ---- velocity, scene-flow and optical-flow maps of an eval-mode render (an addition to ABI v5; csrc/flow.hip; the reference has no counterpart: its
 *      Renderer's `velocity` output is the mask map).  Call after nvfi_render_fwd with the same f, R, rays, t, flags (NVFI_WANT_FLOW set, no
 *      NVFI_TRAIN) and workspace.  Over the appearance-masked samples j of ray r (weight w_j > weight_thres), x_j the UN-warped normalised sample
 *      position at time t, s = aabbSize / 2:
 *        vel_map[r]  (R,3) = sum_j w_j s * v_g(x_j, t)                 v_g: VelocityAABB[Sur].forward, world units per unit time
 *        flow_map[r] (R,3) = sum_j w_j s * (Phi(x_j) - x_j)            Phi(x) = integrate_pos(x, t, t + dt): dt > 0 forward in time, dt == 0 exact zeros
 *        flow2d[r]   (R,2) = sum_j w_j (pi(P'_j) - pi(P_j))            pixels; P = aabb_min + (x + 1) s, pi the inverse of nvfi_gen_rays for the camera
 *                                                                     (pose3x4, H, W, focal); a sample whose displaced point is closer than 1e-3
 *                                                                     in front of the camera contributes nothing; skipped when pose3x4 is NULL
 *      Each output pointer may be NULL.  A ray without masked samples gets zeros.  Ordered sums, no float atomics: repeats bit for bit.  The masked
 *      count never reaches the host.  Errors (2): workspace planned without NVFI_WANT_FLOW, NVFI_TRAIN, use_vel == 0, vel_fp16 modes 1 / 2, a dt
 *      that needs more than 64 RK2 steps.  vel_fp16 bit 3 selects the fp32 MFMA integrator as in nvfi_integrate_pos. */
int nvfi_render_flow(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d,
                     float t, float dt, int flags, const float* weights,
                     const float* pose3x4 /* or NULL */, int H, int W, float focal,
                     float* vel_map, float* flow_map, float* flow2d,   /* each optional */
                     void* workspace, int64_t workspace_bytes, void* stream);
/* ---- per-object layers and the object-selected render of a MaskField decomposition (additions to ABI v5; csrc/objects.hip; the reference has no
 *      counterpart).
 *      nvfi_render_objects: call after nvfi_render_fwd (or nvfi_render_fwd_select) AND nvfi_render_mask with the same f, m, R, t, flags (NVFI_WANT_MASK
 *      set, no NVFI_TRAIN) and workspace.  M_r the appearance-masked samples of ray r (weight w_j > weight_thres), m_jk the softmax nvfi_render_mask
 *      stored, c_j the colour the composite used (MLP_PE and SH shading both), z_j the sample depth, k < mask_dim = K:
 *        obj_acc[r][k]    (R,K)   = sum_{j in M_r} w_j m_jk            the bits of mask_map
 *        obj_rgb[r][k][:] (R,K,3) = sum_{j in M_r} w_j m_jk c_j        premultiplied: no background, no clamp; sum_k = the colour before background / clamp
 *        obj_depth[r][k]  (R,K)   = sum_{j in M_r} w_j m_jk z_j        no (1 - acc) far term
 *      Each output pointer may be NULL.  One pass over a ray's entries gives all 5 K sums; ordered, no float atomics: repeats bit for bit.  A ray
 *      without masked samples gets exact zeros.  The masked count never reaches the host.  Buffers of the workspace the call relies on: the masked
 *      list and its per-ray offsets (mlist, off_m: nvfi_render_fwd), the sample depths (xw.w) and the per-sample colours (rgbs) of that call, and
 *      the per-sample softmax (maskv) nvfi_render_mask wrote.  Whether nvfi_render_mask has run on the workspace cannot be seen from the host
 *      without a synchronisation: the ORDER fwd -> mask -> objects is the caller's duty (without it maskv is stale or uninitialised).
 *      Errors (2): NVFI_TRAIN, flags without NVFI_WANT_MASK, a workspace smaller than the plan of these flags.
 *      nvfi_render_fwd_select: nvfi_render_fwd with, for every valid sample at the warped keyframe position x where its density is looked up,
 *        s(x) = sum_k select[k] * softmax(MaskField(x))_k,   sigma' = sigma * s(x)
 *      and everything downstream unchanged on sigma' (alpha, transmittance, weights, the weight > weight_thres appearance mask, appearance, composite,
 *      depth, acc, background): removing the object in front reveals what is behind it.  select: device float[mask_dim] in [0,1] (1 keeps, 0 removes,
 *      fractions fade); select == NULL is exactly nvfi_render_fwd (same launches, same bits).  Needs NVFI_WANT_SELECT in flags (the room sits behind
 *      everything else: the flag moves no other buffer); eval only: NVFI_TRAIN gives error 2.  use_vel == 0 fields are allowed (x is the sample
 *      position).  Layers of a selected render: nvfi_render_fwd_select -> nvfi_render_mask -> nvfi_render_objects on one workspace. */
int nvfi_render_objects(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, float t, int flags, const float* weights,
                        float* obj_rgb, float* obj_acc, float* obj_depth,   /* each optional */
                        void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_render_fwd_select(const nvfi_field_desc* f, const nvfi_mask_desc* m, const float* select /* or NULL */, int64_t R,
                           const float* rays_o, const float* rays_d, const float* jitter, float t, int flags,
                           float* rgb, float* depth, float* acc, float* weights,
                           void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream);
/* ---- MaskField on free points, forward and backward: the model train_segm.py:126-227 optimises (models/mask_field.py:68-83;
 *      xyz (N,3) -> softmax mask (N,mask_dim)).  mode & NVFI_MASK_TRAIN keeps the activations in `workspace` for nvfi_maskfield_bwd, which
 *      ACCUMULATES d loss / d W_l, b_l (l = point_fc.0..3, mask_fc) from g_mask = d loss / d mask (N,mask_dim); the points carry
 *      no gradient (the reference computes them under no_grad, train_segm.py:137-170). */
typedef struct nvfi_mask_grads { float* W[5]; float* b[5]; } nvfi_mask_grads;
int nvfi_maskfield_workspace_bytes(const nvfi_mask_desc* m, int64_t N, int train, int64_t* bytes);
#define NVFI_MASK_TRAIN 1   /* keep the activations in `workspace` for nvfi_maskfield_bwd */
#define NVFI_MASK_FP16  2   /* layer products on the fp16-input MFMA (weights and layer inputs rounded to fp16, fp32 accumulation,
                               fp32 bias / ReLU / softmax / stashes / weight gradients); default: exact fp32 MFMA */
int nvfi_maskfield_fwd(const nvfi_mask_desc* m, int64_t N, const float* xyz, float* mask_out, int mode,
                       void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_maskfield_bwd(const nvfi_mask_desc* m, int64_t N, const float* g_mask, const nvfi_mask_grads* grads, int mode,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* ---- the objective of the MaskField training step (train_segm.py:182-202; utils/seg_loss.py: dynamic_loss with fit_motion_svd_batch,
 *      smooth_loss, entropy_loss; additions to ABI v5).  pc (N,3) normalised keyframe-0 points, flow (N,3), mask (N,K) the MaskField output,
 *      2 <= K <= 16; everything fp32.  One workspace size serves both calls. */
int nvfi_segloss_workspace_bytes(int64_t N, int K, int k, int64_t* bytes);
/* k nearest points of the SAME cloud for every point (pytorch3d knn_points(pc, pc, K=k) as smooth_loss uses it, seg_loss.py:96-98):
 * idx (N,k) int32 ascending by (squared distance, index), the point itself (or a duplicate of it with a lower index) in slot 0; a slot whose
 * SQUARED distance exceeds `radius` - the reference compares squared distances with its radius - and a slot that does not exist (k > N)
 * holds slot 0's index, d2 (N,k, optional) holds +inf there.  Exact: a cell grid of side >= sqrt(radius), 27 cells per point, no N x N matrix.
 * rev_start (N+1) / rev_edge (N*k) (optional, together): reverse adjacency - the edges e = n*k + j with idx[e] = p != n, for every p the
 * ascending run rev_edge[rev_start[p] .. rev_start[p+1]) (entries from rev_start[N] on are not written) - which nvfi_segloss needs for the
 * smoothness gradient. */
int nvfi_knn_self(int64_t N, const float* pc, int k, float radius, int32_t* idx, float* d2, int32_t* rev_start, int32_t* rev_edge,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* forward and backward of the three losses in one call.  losses4 (device float[4]) receives the UN-weighted dynamic_loss, smooth_loss and
 * entropy_loss as the reference functions return them and, in [3], w_dynamic*[0] + w_smooth*[1] + w_entropy*[2]; gmask (N,K, optional) receives grad_scale * d(w_dynamic*dynamic + w_smooth*smooth +
 * w_entropy*entropy)/d mask (accumulate != 0: is added to).  R (K,3,3), t (K,3): the rigid fit per object (detached, as in seg_loss.py:79:
 * no SVD backward; the identity where the object's S has a NaN), pc_transformed (N,3, optional) = sum_k mask_k (R_k pc + t_k).
 * pc = flow = NULL leaves the rigid-fit term out (losses4[0] = 0), idx = NULL the smoothness term (losses4[1] = 0); loss_norm is 1 or 2. */
int nvfi_segloss(int64_t N, int K, const float* pc, const float* flow, const float* mask, int k, const int32_t* idx,
                 const int32_t* rev_start, const int32_t* rev_edge, int loss_norm, float epsilon, float w_dynamic, float w_smooth,
                 float w_entropy, float grad_scale, int accumulate, float* gmask, float* losses4, float* R, float* t,
                 float* pc_transformed, void* workspace, int64_t workspace_bytes, void* stream);
/* ---- characteristic loss (an addition to ABI v5; csrc/charloss.hip; reference TensorVMKeyframeTimeKplane.characteristic_loss,
 *      models/tensorf_keyframe.py:552-573): features stored at keyframe t_k, read at x, must equal the features of keyframe 0 read where x is
 *      advected back to.  points (N,3) normalised.  t_k = round_half_even(clamp(t / ts, 0, K-1)) * ts for t > 0, else ts = tmax / (K-1) (the
 *      reference's snap); x0 = nvfi_integrate_pos(points, t_k, 0) - the same launch path, x6 by default - written to points0_out when non-NULL.
 *        loss[0] = mean_N (d_t - d_0)^2               d = compute_densityfeature at (points, row k) and at (x0, row 0)
 *        loss[1] = mean_{N x app_dim} (a_t - a_0)^2   a = compute_appfeature (after basis_mat)
 *      Both values are UN-weighted.  grads non-NULL: `weight` x the gradient of loss[0] + loss[1] is ACCUMULATED into grads->dps/dpt/aps/apt/basis
 *      (a NULL member skips that tensor; no other member is read or written: nothing reaches the velocity nets, the warp is a constant as under
 *      the reference's no_grad).  grads == NULL: value only.  t_k == 0: both values are exact zeros, x0 = points, no gradient is touched.
 *      Value and gradients come out of the same pass; plane gradients are float atomics (NVFI_DETERMINISTIC does not cover this call).
 *      Errors (2): N <= 0, use_vel == 0, K < 2, Cd != 24, Ca != 48, app_dim > 32. */
int nvfi_char_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes);
int nvfi_char_loss(const nvfi_field_desc* f, int64_t N, const float* points, float t, float weight,
                   float* loss /* device float[2] */, float* points0_out /* (N,3) or NULL */, const nvfi_grads* grads /* or NULL */,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* SHRender (models/tensorf_model_utils.py:292-296 with models/sh.py:87-110, degree 2): view (N,3), feat (N,27) -> rgb (N,3) */
int nvfi_sh_render(int64_t N, const float* view, const float* feat27, float* rgb, void* stream);

/* ---- per-iteration plane regularisers (next-row f-1): density_L1, TV_loss_density, TV_loss_app
 *      (models/tensorf_keyframe.py:188-231, utils/tensorf_utils.py:139-158) in one pass.  out3 (device float[3]) receives the
 *      UN-weighted values (L1, TV density, TV app) exactly as the reference functions return them; when grads is non-NULL the
 *      gradient of  w_l1*L1 + w_tv_density*TVd + w_tv_app*TVa  is accumulated into grads->dps/dpt/aps. */
int nvfi_plane_regs(const nvfi_field_desc* f, float w_l1, float w_tv_density, float w_tv_app, float* out3,
                    const nvfi_grads* grads, void* stream);
/* same with the three weights read from DEVICE memory (float[3]): the autograd backward of `weight * field.density_L1()` receives its
 * upstream gradient as a device scalar */
int nvfi_plane_regs_dev(const nvfi_field_desc* f, const float* w3_dev, float* out3, const nvfi_grads* grads, void* stream);

/* ---- outer optimiser step: torch.optim.Adam(betas, eps) without amsgrad / weight decay (train_nvfi.py:88-96, 243) over n_tensors
 *      parameter tensors in ONE launch.  `t` is a HOST array; p/g/m/v are device pointers (parameter, gradient, exp_avg, exp_avg_sq),
 *      n elements each, lr the tensor's learning rate; `step` counts from 1 (bias corrections); zero_grad != 0 clears g in the same pass. */
typedef struct nvfi_adam_tensor { float* p; float* g; float* m; float* v; int64_t n; float lr; } nvfi_adam_tensor;
/* F.mse_loss(x, target) of a training batch (train_nvfi.py:159,178) with its gradient in one launch: loss[0] = mean((x - target)^2),
 * grad[i] = 2 (x[i] - target[i]) / n.  One workgroup: n <= 2^22. */
int nvfi_mse(const float* x, const float* target, int64_t n, float* loss, float* grad, void* stream);
/* ---- depth supervision (an addition to ABI v5; csrc/depthloss.hip; reference utils/evaluation_utils.py:8-17 compute_depth_loss(pred, gt)):
 *      with m the counted entries and n_c their number, med = LOWER median (sorted element (n_c - 1) / 2, torch.median's), s = mean|x - med|,
 *      u = (pred - med_p) / (s_p + 1e-6), v = (target - med_t) / (s_t + 1e-6), loss[0] = mean((u - v)^2), UN-scaled.
 *      g_pred[i] = grad_scale * d(loss)/d(pred[i]) with torch's rule for the median (its gradient is spread equally over all entries equal
 *      to it, -0.0 == +0.0), exactly 0 at entries that do not count.  gt_index == NULL: gt is (n); else the target of entry i is gt[gt_index[i]]
 *      (a whole depth image and the pixel_ids nvfi_draw_batch wrote; the indices are not range-checked).  NVFI_DEPTH_SKIP_HOLES: entry i counts
 *      only if its target is finite and > 0.  n_c == 0: loss 0, gradient 0.  A NaN among the counted entries: loss and every counted gradient NaN.
 *      n_counted: device int64[1] or NULL.  One launch of one workgroup, n <= 2^22; up to NVFI_DEPTH_LDS_MAX entries both maps are read once
 *      and kept in LDS, above that every pass streams them.  Sums are fp64 in a fixed order: two calls on the same input give the same bits.
 *      No global atomics, no memset, no host synchronisation.  Errors (2): n <= 0, n > 2^22, a NULL pointer, unknown flags. */
#define NVFI_DEPTH_SKIP_HOLES 1
#define NVFI_DEPTH_LDS_MAX 16384
int nvfi_depth_loss(int64_t n, const float* pred, const float* gt, const int64_t* gt_index, int flags, float grad_scale,
                    float* loss, float* g_pred, int64_t* n_counted, void* stream);
/* ---- distortion loss on the ray weights (an addition to ABI v5; csrc/raydist.hip; Mip-NeRF 360 eq. 15 - the reference has no such term):
 *      the samples of a ray are equally spaced (z_j = t_min + step (j + u)), so in normalised distance every interval has the width
 *      delta = step_size / (far - near) and two midpoints differ by (j - i) delta:
 *        D_r = delta [ sum_i sum_j w_i w_j |i - j| + (1/3) sum_i w_i^2 ],  loss[0] = (1/R) sum_r D_r (UN-scaled),  per_ray[r] = D_r,
 *        g_weights[r][i] = grad_scale [* grad_scale_dev[0]] * (delta / R) [ 2 (A_i + B_i) + (2/3) w_i ],  WRITTEN, not accumulated,
 *        A_i = sum_{j<i} (i - j) w_j, B_i = sum_{j>i} (j - i) w_j (double scans of non-negative terms from either end).
 *      loss, per_ray, g_weights: each may be NULL and is then left out; the others do not change by a bit.  grad_scale_dev: device float[1]
 *      (an upstream gradient that never visits the host) or NULL.  One launch of one wave per ray (any S >= 1: the reverse sweep re-reads the
 *      weights; g_weights must not overlap them) + one launch of one workgroup that sums the R per-ray values (fp64, workspace) in a fixed order: two calls
 *      give the same bits.  No atomics, no memset, no host synchronisation.  R == 0: loss[0] = 0, nothing else is written.
 *      workspace: read and written only when loss is not NULL and R > 0 (it holds the R doubles the mean sums); otherwise it may be NULL.
 *      Errors: 2 (R < 0, S < 1, weights NULL), 4 (a needed workspace that is NULL, smaller than nvfi_ray_distortion_workspace_bytes(R) or not
 *      8-byte aligned), before any launch. */
int nvfi_ray_distortion_workspace_bytes(int64_t R, int64_t* bytes);
int nvfi_ray_distortion(int64_t R, int S, const float* weights /* (R,S) */, float delta,
                        float grad_scale, const float* grad_scale_dev /* device float[1] multiplied in, or NULL */,
                        float* loss /* device float[1], un-scaled mean; or NULL */,
                        float* per_ray /* (R) D_r; or NULL */,
                        float* g_weights /* (R,S), WRITTEN not accumulated: grad_scale [* *grad_scale_dev] * d loss/d w; or NULL */,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* ---- optical-flow supervision of a TRAINING render (an addition to ABI v5; csrc/flowloss.hip; not in the reference - the definition's source is
 *      nvfi_render_flow above): the flow map of a render nvfi_render_fwd* made with NVFI_TRAIN, of R rays at HOST-scalar time t, its loss against
 *      a target flow, and all gradients.
 *        M_r   the appearance-masked samples of ray r: the workspace's mlist / off_m AS THE RENDER MADE THEM (w > weight_thres is not re-evaluated)
 *        w_j   the render's fp32 weights;  z_j the sample depth the render used (xw.w: jitter and the t_min rule are in it)
 *        x_j   = normalize_coord(o_r + d_r z_j), the UN-warped position at time t, fp32;  s = aabbSize / 2
 *        Phi   = integrate_pos(x, t, t + dt) with every rule of nvfi_advect_grad on the uniform schedule; more than 64 steps: error 2; dt == 0: identity
 *        pi    the projection of nvfi_render_flow for the camera (pose3x4 - a DEVICE pointer -, H, W, focal); P = aabb_min + (x + 1) s
 *        a sample whose displaced point has -c_z < 1e-3 contributes nothing, and its gradient is exactly zero.  Only the DISPLACED point is
 *        guarded: a sample whose ORIGINAL point has -c_z == 0 gives a non-finite value (the caller keeps the samples in front of the camera)
 *        flow2d[r] (R,2) = sum_{j in M_r} w_j (pi(P'_j) - pi(P_j))   pixels, an ordered sum: repeats bit for bit
 *        ray r is VALID when (valid == NULL or valid[r] != 0) and both target components are finite; n = the number of valid rays
 *        e_r = flow2d[r] - target[r];  loss = (1 / (2 n)) sum_valid sum_c rho(e_rc);  kind 0: rho(e) = e^2;  kind 1: torch's huber_loss(huber_delta)
 *        element form;  n == 0: loss = 0 and all gradients exactly zero.  The mean is formed in a fixed order with fp64 partials.  n stays on the
 *        device: loss is device float[2] = (loss, n).
 *      Gradients are grad_scale [* grad_scale_dev[0]] times the following, every discrete decision held fixed:
 *        g_weights[r][j] = g_r . (pi(P'_j) - pi(P_j)) for j in M_r, 0 elsewhere; the (R,S) array is WRITTEN, with NVFI_FLOWLOSS_ADD_GW in loss_flags
 *                          ADDED to (composes with the scratch of nvfi_ray_distortion);  g_r = rho'(e_r) / (2 n), 0 for an invalid ray
 *        g_xd[j] = w_j s (.) R_cam Jpi(c'_j)^T g_r, with d = -c_z: du/dc = focal (1/d, 0, c_x/d^2), dv/dc = -focal (0, 1/d, c_y/d^2);  it goes through
 *                          the adjoint of Phi into weight_net (grads->vW / vb, ACCUMULATED) and reaches nothing else: rays, t, dt, the pose, the
 *                          planes and a_weight_net get nothing; no second order.
 *      nvfi_flow_loss_fwd: after the training forward, before its backward.  render_workspace is READ only and left bit-identical; all scratch is
 *      in `workspace` (nvfi_flow_loss_workspace_bytes with the SAME R, t, dt, chunk_cap), which must stay untouched until the last
 *      nvfi_flow_loss_bwd of the call.  loss, flow2d, g_weights: each may be NULL.
 *      nvfi_flow_loss_bwd: the entries [first, first + chunk_cap) of the masked list, clipped on the DEVICE to the masked count, through the chain of
 *      nvfi_advect_grad; call it for first = 0, chunk_cap, 2 chunk_cap, ... < R * n_samples.  A chunk wholly beyond the masked count launches
 *      kernels that exit at once and changes no gradient.  dt == 0: nothing is launched.
 *      No host synchronisation, the masked count never reaches the host, no float atomics outside the weight-gradient reduce.
 *      Errors, before any launch: (2) flags without NVFI_TRAIN, use_vel == 0, vel_fp16 modes 1 / 2, more than 64 RK2 steps, pose3x4 or target NULL,
 *      R <= 0, an unknown kind / loss_flags; (4) a workspace that is NULL, too small or not 16-byte aligned. */
#define NVFI_FLOWLOSS_ADD_GW 1
int nvfi_flow_loss_workspace_bytes(const nvfi_field_desc* f, int64_t R, float t, float dt, int64_t chunk_cap, int64_t* bytes);
int nvfi_flow_loss_fwd(const nvfi_field_desc* f, int64_t R, const float* rays_o, const float* rays_d, float t, float dt, int flags,
                       const float* weights /* (R,S) of the render */,
                       const float* pose3x4, int H, int W, float focal,
                       const float* target /* (R,2) */, const uint8_t* valid /* (R) or NULL */, int kind, float huber_delta,
                       float grad_scale, const float* grad_scale_dev /* device float[1] multiplied in, or NULL */, int loss_flags,
                       float* loss /* device float[2]: un-scaled loss, n; or NULL */, float* flow2d /* (R,2) or NULL */,
                       float* g_weights /* (R,S) or NULL */,
                       const void* render_workspace, int64_t render_workspace_bytes, int64_t chunk_cap,
                       void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_flow_loss_bwd(const nvfi_field_desc* f, int64_t R, float t, float dt, int64_t first, int64_t chunk_cap,
                       const nvfi_grads* grads /* vW / vb ACCUMULATED, the rest ignored */,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* ---- 2-D mask supervision of a render (an addition to ABI v5; csrc/maskloss.hip; not in the reference, which renders the soft label map -
 *      nvfi_render_mask above - but has no loss on it): the mask map of a render nvfi_render_fwd* made, of R rays at HOST-scalar time t, its loss
 *      against per-ray labels or soft targets, and all gradients.  K = m->mask_dim.
 *        M_r   the appearance-masked samples of ray r: the workspace's mlist / off_m AS THE RENDER MADE THEM (w > weight_thres is not re-evaluated)
 *        x_j   the warped keyframe position the render stored (xw[list[i]].xyz): the points k_mask_fwd of nvfi_render_mask reads
 *        w_j   the render's fp32 weights
 *        m_jk  = softmax(MaskField(x_j))_k, the field 3 -> 128 x 4 (ReLU) -> K, 1 <= K <= 32, on the exact-fp32 MFMA (NVFI_MASK_FP16 has no form here)
 *        q[r][k] (R,K) = sum_{j in M_r} w_j m_jk   summed in list order, no float atomics: the BITS nvfi_render_mask gives on the same workspace and
 *                        weights; a ray without masked samples gets exact zeros
 *        targets: with `labels` (device int32 (R)) a label in [0, K) makes y_r one-hot, the label K makes y_r = 0 (background), a negative label
 *                        IGNORES the ray.  A label above K is a caller's error; the labels are device data, the host cannot look at them before a
 *                        launch, so on the device such a ray is IGNORED as well.  With `soft` (device float (R,K)) y_r is the row, and a row with a
 *                        non-finite entry ignores the ray.  Exactly one of the two is given.
 *        n     = the number of rays that are not ignored; it stays on the device: loss is device float[2] = (loss, n)
 *        kind 0 (l2): loss = 1 / (2 n K) sum_valid sum_k (q_rk - y_rk)^2
 *        kind 1 (ce): loss = -(1 / n) sum_valid sum_k y_rk log(q_rk + eps), eps > 0 the caller's; q is NOT renormalised by the ray's opacity; a
 *                        background ray (y = 0) adds nothing to the value or the gradient but counts in n
 *        n == 0: loss = 0 and every gradient exactly zero.  The mean is formed in a fixed order with fp64 partials.
 *      Gradients are grad_scale [* grad_scale_dev[0]] times the following, every discrete decision held fixed:
 *        g_q[r][k]       = (q - y) / (n K) (l2), -y / ((q + eps) n) (ce), 0 for an ignored ray
 *        g_weights[r][j] = sum_k g_q[r][k] m_jk for j in M_r, 0 elsewhere; the (R,S) array is WRITTEN, with NVFI_MASKLOSS_ADD_GW in loss_flags ADDED
 *                          to (composes with the scratch nvfi_ray_distortion and nvfi_flow_loss_fwd share)
 *        g_mask[j][k]    = w_j g_q[ray(j)][k]; it goes through the softmax and MLP adjoint of nvfi_maskfield_bwd into the ten tensors of
 *                          nvfi_mask_grads, ACCUMULATED; a NULL member skips that tensor
 *        Nothing reaches the points x_j (as in nvfi_maskfield_bwd and the host-assembled train-mode mask map): the velocity net and the planes
 *        get something only through g_weights and the render backward.  No second order.
 *      nvfi_mask_loss_fwd: behind nvfi_render_fwd* with the same f, R, t, flags - with NVFI_TRAIN or without (an eval-mode workspace has the same
 *      mlist, off_m and xw); NVFI_WANT_MASK is not required.  render_workspace is READ only and left bit-identical; everything the backward needs
 *      (per entry the position, the ray index and the weight; per ray g_q; the packed forward and transposed fragments; the masked count) is copied
 *      into `workspace` (nvfi_mask_loss_workspace_bytes with the SAME R and chunk_cap), which must stay untouched until the last nvfi_mask_loss_bwd of
 *      the call; those may then run beside or after the render backward.  loss, mask_map, g_weights: each may be NULL.
 *      nvfi_mask_loss_bwd: the entries [first, first + chunk_cap) of the masked list, clipped on the DEVICE to the masked count: the MaskField forward
 *      in stash form, the adjoint, the five weight-gradient jobs with the device count; call it for first = 0, chunk_cap, 2 chunk_cap, ... <
 *      R * n_samples (S = f->n_samples of the forward).  A chunk wholly beyond the masked count launches kernels that exit at once and changes no
 *      gradient.  chunk_cap is a multiple of 128, one workgroup's points.
 *      No host synchronisation, the masked count never reaches the host, every clear is a kernel, no float atomics outside the weight-gradient reduce.
 *      Errors, before any launch: (2) a mask desc that is not 3 -> 128 x 4 -> K <= 32 or lacks a pointer, R <= 0, both or neither of labels / soft, an
 *      unknown kind / loss_flags, eps <= 0 with ce, a chunk_cap that is not a positive multiple of 128, R * n_samples >= 2^31 - 256, NULL weights or
 *      render workspace, NVFI_MASKLOSS_ADD_GW without g_weights; in nvfi_mask_loss_bwd also a `first` that is negative, at or beyond R * S or not a
 *      multiple of chunk_cap, and NULL grads; (4) a workspace that is NULL, too small or not 16-byte aligned.  The render workspace is planned again
 *      from f, R, flags, t: what nvfi_render_fwd* refuses for them (2, 4) is refused here too. */
#define NVFI_MASKLOSS_ADD_GW 1
int nvfi_mask_loss_workspace_bytes(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, int64_t chunk_cap, int64_t* bytes);
int nvfi_mask_loss_fwd(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, float t, int flags,
                       const float* weights /* (R,S) of the render */,
                       const int32_t* labels /* (R) or NULL */, const float* soft /* (R,K) or NULL */, int kind, float eps,
                       float grad_scale, const float* grad_scale_dev /* device float[1] multiplied in, or NULL */, int loss_flags,
                       float* loss /* device float[2]: un-scaled loss, n; or NULL */, float* mask_map /* (R,K) or NULL */,
                       float* g_weights /* (R,S) or NULL */,
                       const void* render_workspace, int64_t render_workspace_bytes, int64_t chunk_cap,
                       void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_mask_loss_bwd(const nvfi_mask_desc* m, int64_t R, int S, int64_t first, int64_t chunk_cap,
                       const nvfi_mask_grads* grads /* W / b ACCUMULATED, NULL members skipped */,
                       void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_adam_step(const nvfi_adam_tensor* t, int n_tensors, float beta1, float beta2, float eps, int64_t step, int zero_grad, void* stream);

/* same step with the per-iteration scalars in DEVICE memory (hipGraph replay): hyper_dev[0] = 1/sqrt(1-beta2^step),
 * hyper_dev[1+k] = lr_k / (1-beta1^step) for tensor k of the table (the values nvfi_adam_step derives on the host; no tensor may be empty) */
int nvfi_adam_step_dev(const nvfi_adam_tensor* t, int n_tensors, float beta1, float beta2, float eps, const float* hyper_dev, int zero_grad, void* stream);

/* ---- building blocks used by train_segm-style callers and by the parity tests */
/* VelBasis.forward (velocity_field.py:69-75): xt (N,4) -> u (N,6)=(v,a); gated!=0: VelocityAABB[Sur].forward -> (N,3) in u (stride 6).
 * Errors, all before anything is launched: (2) use_vel == 0 (the field has no velocity net), component counts / n_samples the kernels are not
 * built for; (4) a workspace under nvfi_vel_workspace_bytes(f, N). */
int nvfi_vel_eval(const nvfi_field_desc* f, int64_t N, const float* xt, float* u6, int gated,
                  void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_vel_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes);
/* integrate_pos (tensorf_keyframe.py:575-611): x (N,3) normalised, t (N), base (N) -> xk (N,3).
 * Errors, all before anything is launched: (2) use_vel == 0, an unsupported descriptor (as nvfi_vel_eval), N >= 2^31 - 256 (chunk the points);
 * (4) a workspace under nvfi_vel_workspace_bytes(f, N). */
int nvfi_integrate_pos(const nvfi_field_desc* f, int64_t N, const float* x, const float* t, const float* base,
                       float* xk, void* workspace, int64_t workspace_bytes, void* stream);
/* ---- differentiable advection (an addition to ABI v5; csrc/advect.hip): the adjoint of xk = integrate_pos(x, t, t_target) for HOST scalar times,
 *      as autograd carries it through the reference's plain torch code (tensorf_keyframe.py:575-611): RK2 midpoint steps of at most ts / 2, the
 *      last one taking the remainder, the gate of VelocityAABB[Sur] tested on the current point and on the midpoint, with the surround box a step
 *      that leaves it rejected - every such decision held fixed.  The forward is nvfi_integrate_pos (t and base filled with the two scalars) and
 *      keeps nothing: this call runs the warp again on the uniform schedule in training form, then the render's unfused adjoint and its weight-
 *      gradient jobs on that stash.
 *        g_x (N,3), WRITTEN (may be NULL): d loss / d x for the upstream g_xk = d loss / d xk.  A point gated at both evaluations of a step passes its
 *        gradient through that step unchanged; a rejected step is the identity.
 *        grads->vW / vb: the gradient of weight_net is ACCUMULATED (a NULL member skips that tensor); no other member is read or written -
 *        a_weight_net and the planes get nothing.
 *      N == 0 or t == t_target: nothing is launched for the net, g_x = g_xk (a copy kernel), 0 is returned.  All launches go to `stream`; no host
 *      synchronisation.  The workspace (caller-allocated; ~10.8 KB per point and RK2 step + 101 MB of slabs: chunk N, chunks accumulate) may be
 *      reused by the next call on the same stream.  Errors (2): use_vel == 0, vel_fp16 modes 1 / 2, more than 64 RK2 steps (refused, not truncated);
 *      (4): workspace too small. */
int nvfi_advect_grad_workspace_bytes(const nvfi_field_desc* f, int64_t N, float t, float t_target, int64_t* bytes);
int nvfi_advect_grad(const nvfi_field_desc* f, int64_t N, const float* x, float t, float t_target,
                     const float* g_xk /* (N,3) */, float* g_x /* (N,3) or NULL, WRITTEN */,
                     const nvfi_grads* grads /* vW / vb ACCUMULATED, the rest ignored */,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* differentiable advection with PER-POINT times (nvfi_advect_pt_steps, nvfi_advect_grad_pt_workspace_bytes, nvfi_advect_grad_pt): declared in
 * nvfi_hip_advect_pt.h, which this line brings in - part of this header for every C consumer.  The prototype list of THIS file is the one
 * nvfi_amd/_lib.py: SIGNATURES restates row by row; additions behind it live in headers of their own, with their rows in _lib.ADDITIONS. */
#include "nvfi_hip_advect_pt.h"
/* compute_densityfeature + feature2density (tensorf_keyframe.py:233-272, 312-321): xyzt (N,4) -> feat (N), sigma (N).
 * Errors (2), before anything is launched: an unsupported descriptor, N >= 2^31 - 256 (chunk the points). */
int nvfi_density_at(const nvfi_field_desc* f, int64_t N, const float* xyzt, float* feat, float* sigma, void* stream);
/* compute_appfeature + MLPRender_PE (tensorf_keyframe.py:274-310, tensorf_base.py:88-98): xyzt (N,4), view (N,3) -> rgb (N,3).
 * Errors, before anything is launched: (2) an unsupported descriptor, N >= 2^31 - 256 (chunk the points); (4) a workspace under
 * nvfi_app_workspace_bytes(f, N). */
int nvfi_app_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes);
int nvfi_app_at(const nvfi_field_desc* f, int64_t N, const float* xyzt, const float* view, float* rgb,
                void* workspace, int64_t workspace_bytes, void* stream);
/* ---- differentiable field lookups (additions to ABI v5; csrc/lookup.hip): compute_densityfeature / compute_appfeature (tensorf_keyframe.py:233-310)
 *      at given points as autograd carries them through the reference's plain torch code - to the six planes of the family, to basis_mat.weight
 *      and to the points themselves, the time coordinate included.  xyzt (N,4): normalised x, y, z and t' (normalize_time_coord(t); per point,
 *      fractional or outside [-1, 1]): every plane, time planes included, takes the four taps of F.grid_sample(align_corners=True,
 *      padding_mode="zeros") on the cell common.h's bl_setup_xy picks from the fp32 coordinates, like nvfi_density_at.
 *        density     feat = sum_c prod_i space_i[c] prod_i time_i[c]; the forward IS nvfi_density_at.
 *        appearance  feat (N, app_dim) = basis_mat (prod_i space_i prod_i time_i).
 *        g_feat      the upstream gradient d loss / d feat: (N) resp. (N, app_dim).
 *        g_xyzt      (N,4), OVERWRITTEN (plain stores; may be NULL): d loss / d (x, y, z, t') - ATen's grid_sampler_2d_backward, the difference of the
 *                    in-range taps times (W - 1) / 2, (H - 1) / 2 and, for t', (K - 1) / 2.  Repeats bit for bit, like feat.
 *        grads       density: dps[3] / dpt[3]; appearance: aps[3] / apt[3] / basis.  ACCUMULATED (+=) into buffers the caller cleared; a NULL
 *                    member (or grads == NULL) skips that tensor; no other member is read.  These are float atomics: they do NOT repeat bit for bit
 *                    and are not covered by NVFI_DETERMINISTIC (2304 B of atomics per point for density, 4608 B for appearance).
 *      The backward reads the taps again: no stash, no workspace, nothing is cleared, one launch on `stream`, no host wait - the calls can be
 *      captured in a hipGraph.  A non-finite or far coordinate has every tap masked: value 0, gradients 0.  N == 0: nothing is launched or
 *      written, 0 is returned.  Errors (2), before anything is launched: an unsupported descriptor, N >= 2^31 - 256 (chunk the points), a NULL
 *      xyzt / g_feat / feat. */
int nvfi_density_grad(const nvfi_field_desc* f, int64_t N, const float* xyzt /* (N,4) normalised x,y,z,t' */,
                      const float* g_feat /* (N) */, float* g_xyzt /* (N,4), OVERWRITTEN, or NULL */,
                      const nvfi_grads* grads /* dps[3], dpt[3] accumulate (+=); NULL pointers skipped */, void* stream);
int nvfi_appfeat_at(const nvfi_field_desc* f, int64_t N, const float* xyzt, float* feat /* (N, app_dim) */, void* stream);
int nvfi_appfeat_grad(const nvfi_field_desc* f, int64_t N, const float* xyzt, const float* g_feat /* (N, app_dim) */,
                      float* g_xyzt /* (N,4) or NULL */, const nvfi_grads* grads /* aps[3], apt[3], basis */, void* stream);
/* renderModule(pts, viewdirs, features) as a stand-alone call - MLPRender_PE.forward (tensorf_base.py:88-98) or, with shading = 1,
 * SHRender (tensorf_model_utils.py:292-296): xyz (N,3) normalised positions, view (N,3), features (N, app_dim) -> rgb (N,3).
 * Workspace: 2 x nvfi_app_workspace_bytes(f, N), and less is refused (4).  Forward only (inside a render the module is differentiated by
 * nvfi_render_bwd).  Errors (2), before anything is launched: an unsupported descriptor, N >= 2^31 - 256 (chunk the points). */
int nvfi_render_mlp(const nvfi_field_desc* f, int64_t N, const float* xyz, const float* view, const float* features, float* rgb,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* ---- differentiable point shading (an addition to ABI v5; csrc/point_shade.hip): the adjoint of rgb = nvfi_render_mlp(xyz, view, features) as
 *      autograd carries it through the reference's plain torch code - MLPRender_PE.forward (tensorf_base.py:88-98: positional encodings of
 *      pts and viewdirs, three Linear layers, ReLU, sigmoid) or, with shading = 1, SHRender (tensorf_model_utils.py:292-296 + sh.py:
 *      relu(sum_k SH_k(view) feat[9c + k] + 0.5)).  Like nvfi_advect_grad the call keeps nothing from the forward: it runs k_app_fwd again in
 *      stash form on the caller's features, then k_pshade_bwd (one 32-point tile per wave on the fp32 MFMA engine) and the render's split-K
 *      weight-gradient jobs on that stash.
 *        g_rgb       (N,3): the upstream gradient d loss / d rgb.  The seeds are g_rgb_c c (1 - c) with c the replayed sigmoid output (MLP_PE),
 *                    resp. g_rgb_c where the replayed colour is > 0 (SH: torch's relu backward).
 *        g_features  (N, app_dim), OVERWRITTEN (plain stores; may be NULL).
 *        g_xyz       (N,3), OVERWRITTEN (may be NULL): the raw slot plus the chain through sin / cos (2^k x); zeros under SH, which does not read xyz.
 *        g_view      (N,3), OVERWRITTEN (may be NULL): the same rule on the view slots; under SH through the derivatives of the nine bases.
 *                    The three per-point outputs repeat bit for bit.
 *        grads       rW[3] / rb[3]: ACCUMULATED (+=, one float atomic per entry and call, from slabs summed in a fixed order: a call into cleared
 *                    buffers repeats bit for bit) into buffers the caller cleared; a NULL member (or grads == NULL) skips that tensor; no other
 *                    member is read.  Ignored under SH (there is no MLP).
 *      All launches go to `stream`, no host wait, nothing is cleared with a memset: the call can be captured in a hipGraph.  N == 0: nothing is
 *      launched or written, 0 is returned.  Workspace (caller-allocated, may be reused by the next call on the same stream): 3 KB of stash and
 *      32 B of packed points per point, 1 KB of ReLU masks per 32-point tile, the weight fragments (0.5 MB) and three slab sets (51 MB) - chunk
 *      a large N; the weight gradients of the chunks accumulate.  Errors, before anything is launched: (2) an unsupported descriptor,
 *      N >= 2^31 - 256, a NULL xyz / view / features / g_rgb; (4) a workspace under nvfi_render_mlp_grad_workspace_bytes(f, N). */
int nvfi_render_mlp_grad_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes);
int nvfi_render_mlp_grad(const nvfi_field_desc* f, int64_t N,
                         const float* xyz /* (N,3) */, const float* view /* (N,3) */, const float* features /* (N, app_dim) */,
                         const float* g_rgb /* (N,3) */,
                         float* g_features /* (N, app_dim) or NULL, OVERWRITTEN */,
                         float* g_xyz /* (N,3) or NULL, OVERWRITTEN */, float* g_view /* (N,3) or NULL, OVERWRITTEN */,
                         const nvfi_grads* grads /* rW[3] / rb[3] ACCUMULATED; NULL members (or grads == NULL) skipped; nothing else read */,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* ---- multi-GPU: rays and collocation points shard over one process per GPU; the ONLY data-path exchange is the sum of the
 *      flat fp32 gradient buffer (the reference has no distributed code: models/ is single-device).  RCCL over xGMI,
 *      loaded lazily with dlopen.  Bootstrap: rank 0 gets a 128-byte id, the host program distributes it, every rank inits.
 *      nvfi_allreduce_grads is in place and asynchronous on `stream`; average != 0 divides by the world size. */
#define NVFI_UNIQUE_ID_BYTES 128
typedef struct nvfi_comm nvfi_comm;
int nvfi_comm_unique_id(void* id128_host);
int nvfi_comm_init(nvfi_comm** comm, int world, int rank, const void* id128_host);
int nvfi_allreduce_grads(nvfi_comm* comm, float* flat_grads, int64_t count, int average, void* stream);
int nvfi_comm_destroy(nvfi_comm* comm);
/* per-kernel-class HIP-event timing for bench.py: enable, run, collect (host arrays of nvfi_prof_nclasses() entries).
 * classes: 0 rk2_fwd 1 rk2_bwd 2 app_fwd 3 app_bwd 4 wgrad 5 pde_fwd 6 pde_bwd 7 density_fwd 8 density_bwd 9 pde_prefilter */
int nvfi_prof_enable(int on);
int nvfi_prof_collect(double* total_ms, int64_t* count);
int nvfi_prof_nclasses(void);
/* compute_alpha (tensorf_keyframe.py:508-537) for a per-call time: xyz (N,3) WORLD coordinates -> normalise, snap to the keyframe
 * (base 0 when transfer), RK2 back-advect, density, alpha = 1-exp(-sigma*length); alpha_out[n] = max(alpha_out[n], alpha) when
 * accumulate_max != 0 (getDenseAlpha's running maximum over the 60 frame times, :476-497), plain store otherwise.  Like the reference's
 * compute_alpha - and unlike the render - a time that is only isclose to its keyframe still takes its (tiny) RK2 step.  workspace_bytes below
 * nvfi_alpha_workspace_bytes(N) is refused with error 4 before anything is launched, whichever integrator the call takes. */
int nvfi_alpha_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes);
int nvfi_compute_alpha(const nvfi_field_desc* f, int64_t N, const float* xyz_world, float t, int transfer, float length,
                       int accumulate_max, float* alpha_out, void* workspace, int64_t workspace_bytes, void* stream);
/* Camera.get_ray_bundle + pixel selection (models/camera.py:112-138,159-172): pose (device float[12], row-major 3x4 c2w),
 * pixel ids (device int64[n], row-major y*W+x) -> rays_o (n,3), rays_d (n,3) */
int nvfi_gen_rays(const float* pose3x4, int H, int W, float focal, int64_t n, const int64_t* pixel_ids, float* rays_o, float* rays_d, void* stream);
/* ---- the random inputs of ONE training iteration in one launch (ABI v5): what train_nvfi.py:150-178 draws per render (a pixel batch of the
 *      posed image: Camera.sample_rays, models/camera.py:159-172) and what NVFi.get_vel_loss draws (models/nvfi.py:44-47: collocation points
 *      uniform in the box, times uniform in [0,1)), from a counter-based generator (Philox4x32-10 keyed by `seed`; counter = element, segment,
 *      iteration): same (seed, iteration) -> same batch, whatever the launch configuration.  Per batch b < n_batches: R pixel indices uniform in
 *      [0, n_pixels) -> rays_o/rays_d[b] gathered from the camera bundle (n_pixels,3), target[b] gathered from target_img (n_pixels,3) or, when
 *      that is NULL, uniform in [0,1) (synthetic benchmark targets); pixel_ids[b] (int64, optional) receives the indices.  P points + times.
 *      The R pixels of a batch are DISTINCT (np.random.choice(replace=False), camera.py:160): pixel r = perm_b(r), a keyed bijection of
 *      [0, n_pixels) (four-round Feistel network, cycle-walked); R > n_pixels is refused like the reference's draw raises. */
typedef struct nvfi_draw_desc {
    uint64_t seed, iteration;
    const uint64_t* iteration_dev;   /* optional: the iteration counter in DEVICE memory (hipGraph replay) */
    int32_t n_batches; int64_t R; int64_t n_pixels;
    const float* bundle_o; const float* bundle_d; const float* target_img;
    float* rays_o[2]; float* rays_d[2]; float* target[2]; int64_t* pixel_ids[2];
    int64_t P; float aabb[6]; float* points; float* t;
} nvfi_draw_desc;
int nvfi_draw_batch(const nvfi_draw_desc* d, void* stream);
/* ---- evaluation metrics on the GPU (additions to ABI v5; csrc/metrics.hip).  Both calls are asynchronous on `stream`, clear what they need with a
 *      kernel, never wait for the device, and repeat bit for bit.  nvfi_metrics_workspace_bytes: kind 0 = nvfi_ssim(B, C, H, W), kind 1 =
 *      nvfi_segm_confusion (B frames, C = K classes; H, W unused).
 * nvfi_ssim (utils/metrics.py:32-99): 11-tap Gaussian window (window11: HOST pointer to the fp32 1-D window), no padding, per channel; pred / gt
 *      are fp32 and addressed by ELEMENT strides (image, channel, row, column), so (B,C,H,W) and channel-last (H,W,C) frames are read in place.
 *      C <= 4, H, W >= 11.  range_mode 0: dynamic range L as given; 1: derived on the device by the reference's rule from max / min of pred over
 *      the whole call (max > 128 -> 255, min < -0.5 -> min_val -1); 2: the same per image.  out (B,2) fp64: mean of the SSIM map, mean of cs = v1/v2.
 * nvfi_segm_confusion: mask (B,N,K) fp32, K <= 32; labels (B,N) int32 in [0,G), G <= 32 -> counts (B,G,K) int64 = pixels with label g whose
 *      argmax_k mask is k (ties: lowest index), conf_sum (B,K) fp64 = sum of mask[n, argmax] over the pixels predicted k, pred_label (B,N) int32
 *      (optional), bad_labels (B) int32 = number of labels outside [0,G).  That is a DEFERRED check: the call cannot see it without waiting, so
 *      such a pixel is counted nowhere (never an out-of-range write) and the caller raises when it reads the results (metric_segm.py). */
int nvfi_metrics_workspace_bytes(int kind, int64_t B, int C, int H, int W, int64_t* bytes);
int nvfi_ssim(int64_t B, int C, int H, int W, const float* pred, const int64_t* pred_strides4, const float* gt, const int64_t* gt_strides4,
              const float* window11, float L, int range_mode, double* out_b2, void* workspace, int64_t workspace_bytes, void* stream);
int nvfi_segm_confusion(int64_t B, int64_t N, int K, int G, const float* mask, const int32_t* labels, int64_t* counts, double* conf_sum,
                        int32_t* pred_label, int32_t* bad_labels, void* workspace, int64_t workspace_bytes, void* stream);
/* The hand-rolled primitives the MLP engine uses instead of libm (engine.h: one-exp2/one-rcp sigmoid, Cody-Waite sin/cos), evaluated
 * element-wise so that tests can bound their error against float64: kind 0 sigmoid, 1 sin, 2 cos, 3 SiLU, 4 SiLU', 5 SiLU''. */
int nvfi_debug_act(int kind, int64_t n, const float* x, float* y, void* stream);
/* MFMA fragment-layout self test: returns max abs error of a 128x128 fp32 layer against a VALU loop (host float*) */
int nvfi_selftest(float* max_err_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
