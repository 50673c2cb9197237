// point_shade.hip - the adjoint of renderModule(pts, viewdirs, features) at caller-chosen points (nvfi_render_mlp_grad, include/nvfi_hip.h): the
// gradient of a loss on the colour of a point with respect to the caller's features, to the positions, to the view directions and to the six
// tensors of renderModule.mlp.  Reference semantics: autograd through models/tensorf_base.py:88-98 (MLPRender_PE.forward) and, with
// shading = 1, models/tensorf_model_utils.py:292-296 + models/sh.py:87-110 (SHRender).
//
// Nothing is kept between the forward (nvfi_render_mlp, which saves no stash) and this call: the forward runs again here in stash form and
// the render's weight-gradient jobs follow on that stash:
//   k_pshade_pack                      (N,3) xyz -> dense float4, the device count of the weight-gradient jobs
//   launch_app_fwd(stash = true)       k_app_fwd<true> on the caller's features (feat_in), per-point view directions: colours, x_in / h1 / h2 rows,
//                                      the ReLU mask words
//   k_pshade_bwd                       the point form of k_app_bwd: seeds straight from g_rgb (no ray, no weight, no rgb_pre clamp), the same three
//                                      transposed layers, then plain stores of g_features / g_xyz / g_view
//   launch_wgrad                       three ring jobs + the slab reduce, ACCUMULATED into grads->rW / rb
// All on the caller's stream, no host synchronisation, no memset.
#include <string.h>
#include "common.h"
#include "render.h"

#define PS_NSLAB 256                             // slab capacity of a weight-gradient job (one per CU), as the render's
#define PS_SLAB_FLOATS (128 * 128 + 128)

struct PshadeArgs {
    nvfi_field_desc f;
    RenderFrags W;
    int64_t N;
    const float* view; const float* feat; const float* g_rgb;
    const float4* rgbs;                          // the replayed colours, dense
    const float* stash_f; float* stash_b; const unsigned* relu_mask;
    float* g_feat; float* g_xyz; float* g_view;
};

// thread i: point i of the dense image; thread 0 also writes the count the weight-gradient jobs read from device memory
__global__ __launch_bounds__(256) void k_pshade_pack(int64_t N, const float* __restrict__ x, float4* __restrict__ xw, int* __restrict__ count) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0) *count = (int)N;
    if (i >= N) return;
    xw[i] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.f);
}

// One 32-point tile per wave, four waves per workgroup (the layout of k_app_fwd, whose stash tile `tile` this wave reads).  A lane beyond N seeds
// exact zeros: its rows of the backward stash add nothing to a weight or bias gradient, and it stores nothing.
__global__ __launch_bounds__(WG_THREADS, 2) void k_pshade_bwd(PshadeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = (int64_t)i < a.N;
    if (f.shading == 1) {
        // SHRender: d pre_c = g_rgb_c where the replayed colour is positive (relu'); d feat[9c + k] = SH_k(view) d pre_c; d view through the
        // derivatives of the nine bases (sh_bases9); xyz is not read.  No MLP: lane (point, h = 0) does the point's work
        if (!active || h) return;
        const size_t p = (size_t)i;
        const float vd[3] = {a.view[3 * p], a.view[3 * p + 1], a.view[3 * p + 2]};
        const float4 c = a.rgbs[p];
        const float cv[3] = {c.x, c.y, c.z};
        float gpre[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gpre[k] = cv[k] > 0.f ? a.g_rgb[3 * p + k] : 0.f;
        if (a.g_feat) {
            float sh[9];
            sh_bases9(vd, sh);
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3)
#pragma unroll
                for (int k = 0; k < 9; ++k) a.g_feat[27 * p + 9 * c3 + k] = sh[k] * gpre[c3];
        }
        if (a.g_view) {
            const float C1 = 0.4886025119029199f;
            const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
            float B[9];     // d loss / d SH_k
#pragma unroll
            for (int k = 0; k < 9; ++k) B[k] = gpre[0] * a.feat[27 * p + k] + gpre[1] * a.feat[27 * p + 9 + k] + gpre[2] * a.feat[27 * p + 18 + k];
            const float x = vd[0], y = vd[1], z = vd[2];
            a.g_view[3 * p] = -C1 * B[3] + C2[0] * y * B[4] - 2.f * C2[2] * x * B[6] + C2[3] * z * B[7] + 2.f * C2[4] * x * B[8];
            a.g_view[3 * p + 1] = -C1 * B[1] + C2[0] * x * B[4] + C2[1] * z * B[5] - 2.f * C2[2] * y * B[6] - 2.f * C2[4] * y * B[8];
            a.g_view[3 * p + 2] = C1 * B[2] + C2[1] * y * B[5] + 4.f * C2[2] * z * B[6] + C2[3] * x * B[7];
        }
        if (a.g_xyz) { a.g_xyz[3 * p] = 0.f; a.g_xyz[3 * p + 1] = 0.f; a.g_xyz[3 * p + 2] = 0.f; }
        return;
    }
    const float* stf = a.stash_f + (size_t)tile * (APP_F_ROWS * REGF);
    float* stb = a.stash_b + (size_t)tile * (APP_B_ROWS * REGF);
    float g[64];
    f32x16 acc[4];
    // seeds: go_c = g_rgb_c * c (1 - c) in rows 0..2 of a D tile (lane h = 0, registers 0..2)
    {
        float go[3] = {0.f, 0.f, 0.f};
        if (active && h == 0) {
            const float4 c = a.rgbs[i];
            const float cv[3] = {c.x, c.y, c.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) go[k] = a.g_rgb[3 * (size_t)i + k] * cv[k] * (1.f - cv[k]);
        }
        g[0] = go[0]; g[1] = go[1]; g[2] = go[2]; g[3] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) STASH_ST(stb[s * REGF + lane], s < 3 ? g[s] : 0.f);
    }
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t3, RT_3, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 4>(lds_w, lane, g, acc);
    relu_mask_apply(a.relu_mask + (size_t)tile * 256 + 128, lane, acc, g);
    stash_store<64>(stb + 16 * REGF, lane, g);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t2, RT_2, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 64>(lds_w, lane, g, acc);
    relu_mask_apply(a.relu_mask + (size_t)tile * 256, lane, acc, g);
    stash_store<64>(stb + 80 * REGF, lane, g);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t1, RT_1, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 64>(lds_w, lane, g, acc);
    // acc = gradient wrt the 110 input slots (RENDER_IN layout): tile 0 the features, slots 16..18 raw view (h = 0) | raw pts (h = 1),
    // 19..36 sin | cos of pts, 37..54 sin | cos of view
    if (active && a.g_feat) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < f.app_dim) a.g_feat[(size_t)i * f.app_dim + row] = acc[0][r];
        }
    }
    const float* xin = stf + 32 * REGF;
    float gp[3], gv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float sp = h ? acc[1][c] : 0.f, sv = h ? 0.f : acc[1][c];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int slp = 19 + c * 6 + k, slv = 37 + c * 6 + k;
            const float fr = (float)(1 << k);
            // d sin = fr * cos, d cos = -fr * sin: the partner half holds the other function of the pair
            const float op = __shfl_xor(STASH_LD(xin[slp * REGF + lane]), 32);
            const float ov = __shfl_xor(STASH_LD(xin[slv * REGF + lane]), 32);
            sp += (h ? -fr * op : fr * op) * acc[slp >> 4][slp & 15];
            sv += (h ? -fr * ov : fr * ov) * acc[slv >> 4][slv & 15];
        }
        sp += __shfl_xor(sp, 32); sv += __shfl_xor(sv, 32);
        gp[c] = sp; gv[c] = sv;
    }
    if (active && h == 0) {
        const size_t p = (size_t)i;
        if (a.g_xyz) { a.g_xyz[3 * p] = gp[0]; a.g_xyz[3 * p + 1] = gp[1]; a.g_xyz[3 * p + 2] = gp[2]; }
        if (a.g_view) { a.g_view[3 * p] = gv[0]; a.g_view[3 * p + 1] = gv[1]; a.g_view[3 * p + 2] = gv[2]; }
    }
}

struct PshadePlan {
    int64_t cap_tiles, total;
    int* count; float* frag; float4 *xw, *rgbs; float *app_f, *app_b; unsigned* relu; float* slabs;
};
// sized like plan_render's training block: whole 128-point workgroups of stash tiles; the slabs only where there is an MLP
static void plan_pshade(const nvfi_field_desc* f, int64_t N, void* ws, PshadePlan* P) {
    Bump B{(char*)ws, 0, 0};
    P->cap_tiles = (N + WG_SAMPLES - 1) / WG_SAMPLES * 4;
    P->count = B.take<int>(16);
    P->frag = B.take<float>(RENDER_FRAG_FLOATS);
    P->xw = B.take<float4>(N);
    P->rgbs = B.take<float4>(N);
    P->app_f = B.take<float>(P->cap_tiles * (int64_t)(APP_F_ROWS * REGF));
    P->app_b = B.take<float>(P->cap_tiles * (int64_t)(APP_B_ROWS * REGF));
    P->relu = B.take<unsigned>(P->cap_tiles * (int64_t)256);
    P->slabs = f->shading == 0 ? B.take<float>((int64_t)PS_NSLAB * PS_SLAB_FLOATS * 3) : nullptr;
    P->total = align_up(B.off, 256);
}

static int pshade_check(const nvfi_field_desc* f, int64_t N) {
    if (check_desc(f)) return 2;
    if (N >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "nvfi_render_mlp_grad: N too large for one call; chunk the points");
    return 0;
}

extern "C" int nvfi_render_mlp_grad_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes) {
    if (int rc = pshade_check(f, N)) return rc;
    PshadePlan P; plan_pshade(f, N > 0 ? N : 0, nullptr, &P);
    *bytes = N > 0 ? P.total : 256;
    return 0;
}

extern "C" int nvfi_render_mlp_grad(const nvfi_field_desc* f, int64_t N, const float* xyz, const float* view, const float* features,
                                    const float* g_rgb, float* g_features, float* g_xyz, float* g_view, const nvfi_grads* grads,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pshade_check(f, N)) return rc;
    if (N <= 0) return 0;
    if (!xyz || !view || !features || !g_rgb) return nvfi_fail(2, "nvfi_render_mlp_grad: xyz, view, features and g_rgb must be non-NULL");
    PshadePlan P; plan_pshade(f, N, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld bytes, got %lld", (long long)P.total, (long long)workspace_bytes);
    static DeviceOnce once;
    if (once.lds(ENGINE_LDS_BYTES, k_pshade_bwd)) return 1;
    PackJobs jobs; jobs.n = 0; RenderFrags RW;
    if (pack_render_frags(f, P.frag, &RW, &jobs)) return 3;
    if (launch_pack(jobs, st)) return 1;
    hipLaunchKernelGGL(k_pshade_pack, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, xyz, P.xw, P.count);
    LAUNCHCK();
    // the forward again, in stash form
    AppArgs aa; memset(&aa, 0, sizeof(aa));
    aa.f = *f; aa.W = RW; aa.count = nullptr; aa.n_direct = N; aa.list = nullptr; aa.xw = P.xw;
    aa.per_point_t = 1; aa.S = 1; aa.view_per_point = view; aa.rgbs = P.rgbs; aa.rgb_dense = 1; aa.feat_in = features;
    aa.stash_f = P.app_f; aa.stash_b = P.app_b; aa.relu_mask = P.relu;
    if (launch_app_fwd(aa, N, true, st)) return 1;
    PshadeArgs pa; memset(&pa, 0, sizeof(pa));
    pa.f = *f; pa.W = RW; pa.N = N; pa.view = view; pa.feat = features; pa.g_rgb = g_rgb; pa.rgbs = P.rgbs;
    pa.stash_f = P.app_f; pa.stash_b = P.app_b; pa.relu_mask = P.relu; pa.g_feat = g_features; pa.g_xyz = g_xyz; pa.g_view = g_view;
    hipLaunchKernelGGL(k_pshade_bwd, dim3((unsigned)((N + WG_SAMPLES - 1) / WG_SAMPLES)), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, pa);
    LAUNCHCK();
    if (f->shading != 0 || !grads) return 0;
    // render-MLP weight gradients: the render's three jobs (render.hip) on this call's stash
    WgradJobs wj; wj.n = 0; ReduceJobs rj; rj.n = 0;
    const size_t fs = APP_F_ROWS * REGF, bs = APP_B_ROWS * REGF;
    auto add = [&](const float* A, int a_regs, const float* B, int b_regs, float* slabs, float* gW, float* gb, int out, int in, int sk) {
        WgradJob& J = wj.j[wj.n++];
        memset(&J, 0, sizeof(J));
        J.A = A; J.a_tile_stride = bs; J.a_regs = a_regs; J.B = B; J.B2 = nullptr; J.b_tile_stride = fs; J.b_regs = b_regs;
        J.bmode = BM_RAW; J.count = P.count; J.cap_tiles = (int)P.cap_tiles; J.nrep = 1; J.a_rep_stride = 0; J.b_rep_stride = 0;
        J.slabs = slabs; J.nslab = PS_NSLAB;
        ReduceJob& Q = rj.j[rj.n++];
        memset(&Q, 0, sizeof(Q));
        Q.slabs = slabs; Q.nslab = PS_NSLAB; Q.MTA = a_regs / 16; Q.KTB = b_regs / 16; Q.gW = gW; Q.gb = gb; Q.out = out; Q.in = in;
        Q.row_kind = RK_NATURAL; Q.slot_kind = sk; Q.scale = 1.f;
    };
    float* sl = P.slabs;
    const size_t set = (size_t)PS_NSLAB * PS_SLAB_FLOATS;
    if (grads->rW[2] || grads->rb[2]) add(P.app_b + 0, 16, P.app_f + 160 * REGF, 64, sl + 0 * set, grads->rW[2], grads->rb[2], 3, 128, SK_HIDDEN);
    if (grads->rW[1] || grads->rb[1]) add(P.app_b + 16 * REGF, 64, P.app_f + 96 * REGF, 64, sl + 1 * set, grads->rW[1], grads->rb[1], 128, 128, SK_HIDDEN);
    if (grads->rW[0] || grads->rb[0]) add(P.app_b + 80 * REGF, 64, P.app_f + 32 * REGF, 64, sl + 2 * set, grads->rW[0], grads->rb[0], 128, 110, SK_RENDER_IN);
    return launch_wgrad(wj, rj, st);
}
