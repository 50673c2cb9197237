// maskloss.hip - 2-D mask supervision of a render (nvfi_mask_loss_fwd / nvfi_mask_loss_bwd, include/nvfi_hip.h; the reference renders the soft
// label map, tensorf_keyframe.py:749-753, but has no loss on it): the mask map of the render's own appearance-masked samples, its l2 or
// cross-entropy loss against per-ray labels or soft targets, and all gradients - the weights' for the render backward (g_weights), the MaskField's
// ten tensors through the softmax / MLP adjoint of mask.hip.
//
// nvfi_mask_loss_fwd runs behind nvfi_render_fwd* (training or eval flags).  It reads the render workspace READ-ONLY (mlist, off_m, the device
// count, xw.xyz); everything it writes lives in the call's own workspace:
//   launch_pack       the MaskField's forward and transposed fragments (mask.hip's layout)
//   k_ml_fwd<false>   k_mask_fwd's data flow over the masked list: the softmax of every entry (cap x 32 floats, like the render's maskv) + the
//                     entry's position, weight and ray index and the masked count for the backward
//   k_ml_ray          one wave per ray, lanes as in k_mask_final: q[r] as an ordered sum (the bits of nvfi_render_mask), the ray's loss term (fp64)
//   k_ml_mean         ONE workgroup: the valid count n and the mean in a fixed order (reduce.h's ordered workgroup sum)
//   k_ml_grad         one wave per ray: g_q (both depend on n) and g_weights (written behind a zero fill, or added to)
// nvfi_mask_loss_bwd handles the entries [first, first + chunk_cap) of the masked list, clipped on the device:
//   k_ml_fwd<true>    the MaskField forward of the chunk in k_maskfield_fwd<true>'s stash layout, + the chunk's device count
//   k_ml_adj          k_maskfield_bwd's adjoint with g_mask[j][k] = w_j g_q[ray(j)][k] formed in registers
//   launch_wgrad      the five weight-gradient jobs of nvfi_maskfield_bwd on the device count
// fp32 MFMA only (engine.h, like k_mask_fwd): no 16-bit matrix instruction is issued here, so the unit needs no packed-fp32 fence.  No host
// synchronisation, no float atomics outside the weight-gradient reduce: two calls repeat bit for bit.
#include <string.h>
#include "reduce.h"
#include "render.h"
#include "maskmlp.h"       // stash rows, fragment sizes and order, slab room: the ones of mask.hip, whose wgrad jobs the chunks run

#define ML_MEAN_THREADS 1024
#define ML_HDR_INTS 16                 // [0] masked count (clipped to the capacity), [1] n, the number of rays that are not ignored

struct MlPlan {
    int* hdr; double* lterm; int* vflag; float* gq;
    float4* pxw; int* ray; float* maskv; float* frag;
    int* ccount; unsigned* relu; float* stash_f; float* stash_b; float* slabs;
    int64_t tiles;                     // stash tiles of one chunk
    int64_t total;
};

struct MlArgs {
    MkFrags W; int K; int S; int64_t R; int64_t cap;
    const int* count; const int* off_m; const int* list; const float4* xw; const float* weight;
    int* hdr; double* lterm; int* vflag; float* gq;
    float4* pxw; int* ray; float* maskv;
    const int* labels; const float* soft; int kind; float eps;
    float grad_scale; const float* grad_scale_dev; int add_gw;
    float* loss; float* mask_map; float* g_weights;
    int64_t first; int64_t chunk_cap;
    int* ccount; unsigned* relu; float* stash_f; float* stash_b;
};

static void plan_mask_loss(int64_t R, int S, int64_t chunk_cap, void* ws, MlPlan* P) {
    Bump B{(char*)ws, 0, 0};
    const int64_t cap = R * (int64_t)S;
    P->hdr = B.take<int>(ML_HDR_INTS);
    P->lterm = B.take<double>(R);
    P->vflag = B.take<int>(R);
    P->gq = B.take<float>(R * 32);
    P->pxw = B.take<float4>(cap);
    P->ray = B.take<int>(cap);
    P->maskv = B.take<float>(cap * 32);
    P->frag = B.take<float>(MK_FRAG_FLOATS);
    P->tiles = chunk_cap / WG_SAMPLES * 4;
    P->ccount = B.take<int>(16);
    P->relu = B.take<unsigned>(P->tiles * (int64_t)MK_MASK_WORDS);
    P->stash_f = B.take<float>(P->tiles * (int64_t)(MK_F_ROWS * REGF));
    P->stash_b = B.take<float>(P->tiles * (int64_t)(MK_B_ROWS * REGF));
    P->slabs = B.take<float>((int64_t)MK_NSLAB * MK_SLAB_FLOATS * 5);
    P->total = align_up(B.off, 256);
}

// the entries a launch over [first, first + cap_n) of the masked list owns
__device__ __forceinline__ int ml_chunk_count(const int* hdr, int64_t first, int64_t cap_n) {
    const int64_t left = (int64_t)hdr[0] - first;
    return (int)(left <= 0 ? 0 : (left > cap_n ? cap_n : left));
}

// STASH = false: the whole masked list of the render (list / xw), the softmax into maskv, + what the backward needs of every entry.
// STASH = true: the chunk [first, first + chunk_cap) of the positions the first form kept, in k_maskfield_fwd<true>'s stash layout.
// The arithmetic is k_mask_fwd's / k_maskfield_fwd's, instruction for instruction: the same bits.
template <bool STASH>
__global__ __launch_bounds__(WG_THREADS, 2) void k_ml_fwd(MlArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    int count;
    if (STASH) {
        count = ml_chunk_count(a.hdr, a.first, a.chunk_cap);
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.ccount = count;
    } else {
        count = (int64_t)*a.count < a.cap ? *a.count : (int)a.cap;
        if (blockIdx.x == 0 && threadIdx.x == 0) a.hdr[0] = count;
    }
    if ((int)(blockIdx.x * WG_SAMPLES) >= count) return;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = i < count;
    float4 q = zero4();
    if (active) {
        if (STASH) q = a.pxw[a.first + i];
        else {
            const int n = a.list[i];
            q = a.xw[n];
            if (h == 0) { a.pxw[i] = make_float4(q.x, q.y, q.z, a.weight[n]); a.ray[i] = n / a.S; }
        }
    }
    float* st = STASH ? a.stash_f + (size_t)tile * (MK_F_ROWS * REGF) : nullptr;
    unsigned* rm = STASH ? a.relu + (size_t)tile * MK_MASK_WORDS : nullptr;
    float xa[64], xb[64];
    xb[0] = h ? q.y : q.x; xb[1] = h ? 0.f : q.z;
    if (STASH) {
#pragma unroll
        for (int s = 0; s < 16; ++s) st[s * REGF + lane] = s < 2 ? xb[s] : 0.f;
    }
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f[0], MK_F0, a.W.b[0], 128);
    __syncthreads();
    layer_tiles<4, 2>(lds_w, lds_b, true, lane, h, xb, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { xa[16 * m + r] = fmaxf(acc[r], 0.f); if (STASH) st[(16 + 16 * m + r) * REGF + lane] = xa[16 * m + r]; }
    });
    if (STASH) relu_mask_store(rm, lane, xa);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f[1], MK_FH, a.W.b[1], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xa, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { xb[16 * m + r] = fmaxf(acc[r], 0.f); if (STASH) st[(80 + 16 * m + r) * REGF + lane] = xb[16 * m + r]; }
    });
    if (STASH) relu_mask_store(rm + 128, lane, xb);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f[2], MK_FH, a.W.b[2], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xb, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { xa[16 * m + r] = fmaxf(acc[r], 0.f); if (STASH) st[(144 + 16 * m + r) * REGF + lane] = xa[16 * m + r]; }
    });
    if (STASH) relu_mask_store(rm + 256, lane, xa);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f[3], MK_FH, a.W.b[3], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xa, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { xb[16 * m + r] = fmaxf(acc[r], 0.f); if (STASH) st[(208 + 16 * m + r) * REGF + lane] = xb[16 * m + r]; }
    });
    if (STASH) relu_mask_store(rm + 384, lane, xb);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f[4], MK_F4, a.W.b[4], 32);
    __syncthreads();
    float o[16];
    layer_tiles<1, 64>(lds_w, lds_b, true, lane, h, xb, [&](int, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = acc[r];
    });
    // softmax over the K logits of the entry: rows (r&3)+8(r>>2)+4h live in this lane, the rest in lane^32
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int row = (r & 3) + 8 * (r >> 2) + 4 * h; if (row < a.K) mx = fmaxf(mx, o[r]); }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int row = (r & 3) + 8 * (r >> 2) + 4 * h; o[r] = row < a.K ? expf(o[r] - mx) : 0.f; sum += o[r]; }
    sum += __shfl_xor(sum, 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float p = o[r] / sum;
        if (STASH) st[(272 + r) * REGF + lane] = p;
        else if (active && row < a.K) a.maskv[(size_t)i * 32 + row] = p;
    }
}

// the target of ray r in channel k and whether the ray counts.  labels: [0, K) one-hot, K background (all zero), anything else ignored;
// soft: the row, ignored when one of its K entries is not finite (every lane of the wave calls this)
__device__ __forceinline__ float ml_target(const MlArgs& a, int64_t r, int k, bool& ok) {
    if (a.labels) {
        const int lab = a.labels[r];
        ok = lab >= 0 && lab <= a.K;
        return (k < a.K && k == lab) ? 1.f : 0.f;
    }
    const float y = k < a.K ? a.soft[r * a.K + k] : 0.f;
    ok = __all(isfinite(y) ? 1 : 0) != 0;
    return y;
}

// one wave per ray; lane = (entry parity e, channel k of 32) as in k_mask_final: two entries per pass, every lane adds its own entries in list
// order, then the two parities are added - the bits of mask_map
__global__ __launch_bounds__(256) void k_ml_ray(MlArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;                              // (whole waves leave: the shuffles below see full waves)
    const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
    const int k = lane & 31, e0 = lane >> 5;
    float s = 0.f;
    for (int i = b0 + e0; i < b1; i += 2) s += a.pxw[i].w * (k < a.K ? a.maskv[(size_t)i * 32 + k] : 0.f);
    s += __shfl_xor(s, 32);
    if (lane < a.K && a.mask_map) a.mask_map[r * a.K + lane] = s;
    if (e0 == 0) a.gq[r * 32 + k] = s;                 // q, until k_ml_grad turns it into g_q
    bool ok;
    const float y = ml_target(a, r, k, ok);
    float term = 0.f;
    if (a.kind == 0) { const float d = s - y; term = d * d; }
    else if (y != 0.f) term = -(y * logf(s + a.eps));
    const double tsum = wave_sum((ok && e0 == 0 && k < a.K) ? (double)term : 0.0);
    if (lane == 0) { a.lterm[r] = tsum; a.vflag[r] = ok ? 1 : 0; }
}

// n = number of rays that count, loss = sum of the per-ray terms / (2 n K) (l2) or / n (ce): every thread sums its stride, then the workgroup's
// ordered sums (reduce.h)
__global__ __launch_bounds__(ML_MEAN_THREADS) void k_ml_mean(MlArgs a) {
    __shared__ double part[ML_MEAN_THREADS / 64];
    __shared__ int npart[ML_MEAN_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int64_t i = tid; i < a.R; i += ML_MEAN_THREADS) { s += a.lterm[i]; n += a.vflag[i]; }
    block_sum_ordered<ML_MEAN_THREADS / 64, 1>(&s, part, tid & 63, tid >> 6);
    block_sum_ordered<ML_MEAN_THREADS / 64, 1>(&n, npart, tid & 63, tid >> 6);
    if (tid == 0) {
        a.hdr[1] = n;
        if (a.loss) {
            const double den = a.kind == 0 ? 2.0 * (double)n * (double)a.K : (double)n;
            a.loss[0] = n > 0 ? (float)(s / den) : 0.f; a.loss[1] = (float)n;
        }
    }
}

// one wave per ray, lanes as in k_ml_ray: g_q[r][k] in place of q, then per entry g_weights = sum_k g_q[k] m_jk as a fixed butterfly over the
// 32 channel lanes of the entry's parity
__global__ __launch_bounds__(256) void k_ml_grad(MlArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
    const int k = lane & 31, e0 = lane >> 5;
    const int nv = a.hdr[1];
    const float q = a.gq[r * 32 + k];
    bool ok;
    const float y = ml_target(a, r, k, ok);
    ok = ok && a.vflag[r] != 0 && nv > 0;
    float g = 0.f;
    if (ok && k < a.K) {
        const double sc = (double)a.grad_scale * (a.grad_scale_dev ? (double)a.grad_scale_dev[0] : 1.0) / (double)nv;
        if (a.kind == 0) g = (float)(sc / (double)a.K * (double)(q - y));
        else if (y != 0.f) g = (float)(-sc * (double)(y / (q + a.eps)));
    }
    if (e0 == 0) a.gq[r * 32 + k] = g;
    if (!a.g_weights) return;
    for (int i0 = b0; i0 < b1; i0 += 2) {              // (uniform trip count: the shuffles see full waves)
        const int i = i0 + e0;
        const bool in = i < b1;
        float v = (in && k < a.K) ? g * a.maskv[(size_t)i * 32 + k] : 0.f;
        v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
        if (in && k == 0) {
            const int n = a.list[i];
            if (a.add_gw) a.g_weights[n] += v; else a.g_weights[n] = v;
        }
    }
}

// adjoint of the chunk (k_maskfield_bwd on the chunk's stash): g_mask[j][k] = w_j g_q[ray(j)][k], g_logits = p * (g - sum_k g_k p_k), then
// g_z_l = (W_{l+1}^T g_z_{l+1}) * [h_l > 0].  Nothing goes on to the points.
__global__ __launch_bounds__(WG_THREADS, 2) void k_ml_adj(MlArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int count = ml_chunk_count(a.hdr, a.first, a.chunk_cap);
    if ((int)(blockIdx.x * WG_SAMPLES) >= count) return;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = i < count;
    const float* stf = a.stash_f + (size_t)tile * (MK_F_ROWS * REGF);
    float* stb = a.stash_b + (size_t)tile * (MK_B_ROWS * REGF);
    const unsigned* rm = a.relu + (size_t)tile * MK_MASK_WORDS;
    float g[64];
    {
        const float w = active ? a.pxw[a.first + i].w : 0.f;
        const float* gq = a.gq + (size_t)(active ? a.ray[a.first + i] : 0) * 32;
        float p[16], go[16], dot = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            p[r] = stf[(272 + r) * REGF + lane];
            go[r] = (active && row < a.K) ? w * gq[row] : 0.f;
            dot += go[r] * p[r];
        }
        dot += __shfl_xor(dot, 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) { g[r] = p[r] * (go[r] - dot); stb[r * REGF + lane] = g[r]; }
    }
    f32x16 acc[4];
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t[4], MK_T4, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 16>(lds_w, lane, g, acc);
#pragma unroll 1
    for (int l = 3; l >= 1; --l) {
        float* gz = stb + (size_t)(16 + 64 * (3 - l)) * REGF;
        relu_mask_apply(rm + 128 * l, lane, acc, g);
        stash_store<64>(gz, lane, g);
        __syncthreads();
        stage_frag(lds_w, lds_b, a.W.t[l], MK_FH, nullptr, 0);
        __syncthreads();
        acc_init<4>(acc, lds_b, 0, false);
        layer_mfma<4, 64>(lds_w, lane, g, acc);
    }
    {
        float* gz = stb + (size_t)(16 + 64 * 3) * REGF;
        relu_mask_apply(rm, lane, acc, g);
        stash_store<64>(gz, lane, g);
    }
}

// ---------------------------------------------------------------- host
static int ml_mask_check(const char* who, const nvfi_mask_desc* m) {
    if (!m) return nvfi_fail(2, "%s: the mask desc must not be NULL", who);
    if (m->n_layer != 4 || m->n_dim != 128 || m->mask_dim < 1 || m->mask_dim > 32)
        return nvfi_fail(2, "%s: mask field must be 3->128x4->mask_dim<=32 (train_segm.py:97-102); got n_layer=%d n_dim=%d mask_dim=%d", who, m->n_layer, m->n_dim, m->mask_dim);
    for (int l = 0; l < 5; ++l) if (!m->W[l] || !m->b[l]) return nvfi_fail(2, "%s: mask field layer %d has no weight/bias pointer", who, l);
    return 0;
}
static int ml_shape_check(const char* who, int64_t R, int S, int64_t chunk_cap) {
    if (R <= 0) return nvfi_fail(2, "%s: R=%lld, at least one ray is needed", who, (long long)R);
    if (S < 1 || R * (int64_t)S >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "%s: R * n_samples = %lld is more than one call holds", who, (long long)(R * (int64_t)S));
    if (chunk_cap < WG_SAMPLES || chunk_cap % WG_SAMPLES) return nvfi_fail(2, "%s: chunk_cap=%lld must be a positive multiple of %d", who, (long long)chunk_cap, WG_SAMPLES);
    return 0;
}
static int ml_ws_check(const char* who, const MlPlan& P, const void* ws, int64_t ws_bytes) {
    if (!ws || ws_bytes < P.total) return nvfi_fail(4, "%s: workspace of %lld bytes, %lld needed", who, (long long)(ws ? ws_bytes : 0), (long long)P.total);
    if ((uintptr_t)ws & 15) return nvfi_fail(4, "%s: the workspace must be 16-byte aligned", who);
    return 0;
}
// the fragments in the workspace (mk_frag_ptrs: the layout of mask.hip's mask_frags); m != NULL: the pack jobs too
static void ml_frags(const nvfi_mask_desc* m, float* frag, MkFrags* W, PackJobs* jobs) {
    mk_frag_ptrs(frag, W);
    if (!jobs) return;
    jobs->n = 0;
    for (int l = 0; l < 5; ++l) {
        PackJob& J = jobs->j[jobs->n++];
        memset(&J, 0, sizeof(J));
        J.W = m->W[l]; J.b = m->b[l]; J.frag = const_cast<float*>(W->f[l]); J.bfrag = const_cast<float*>(W->b[l]);
        J.out = l < 4 ? 128 : m->mask_dim; J.in = l == 0 ? 3 : 128; J.MT = l < 4 ? 4 : 1; J.NS = l == 0 ? 2 : 64;
        J.row_kind = RK_NATURAL; J.slot_kind = l == 0 ? SK_XYZ : SK_HIDDEN;
    }
    for (int l = 1; l < 5; ++l) {           // dgrad fragments: rows = input features of layer l, slots = its output rows
        PackJob& J = jobs->j[jobs->n++];
        memset(&J, 0, sizeof(J));
        J.W = m->W[l]; J.frag = const_cast<float*>(W->t[l]);
        J.out = l < 4 ? 128 : m->mask_dim; J.in = 128; J.MT = 4; J.NS = l < 4 ? 64 : 16;
        J.row_kind = RK_NATURAL; J.slot_kind = SK_HIDDEN; J.transposed = 1;
    }
}
static int ml_attrs() {
    static DeviceOnce once;
    return once.lds(ENGINE_LDS_BYTES, k_ml_fwd<true>, k_ml_fwd<false>, k_ml_adj);
}

extern "C" int nvfi_mask_loss_workspace_bytes(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, int64_t chunk_cap, int64_t* bytes) {
    const char* who = "nvfi_mask_loss_workspace_bytes";
    if (!f || !bytes) return nvfi_fail(2, "%s: f and bytes must not be NULL", who);
    if (int rc = ml_mask_check(who, m)) return rc;
    if (int rc = ml_shape_check(who, R, f->n_samples, chunk_cap)) return rc;
    MlPlan P;
    plan_mask_loss(R, f->n_samples, chunk_cap, nullptr, &P);
    *bytes = P.total;
    return 0;
}

extern "C" int nvfi_mask_loss_fwd(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, float t, int flags, const float* weights,
                                  const int32_t* labels, const float* soft, int kind, float eps,
                                  float grad_scale, const float* grad_scale_dev, int loss_flags,
                                  float* loss, float* mask_map, float* g_weights,
                                  const void* render_workspace, int64_t render_workspace_bytes, int64_t chunk_cap,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "nvfi_mask_loss_fwd";
    hipStream_t st = (hipStream_t)stream;
    if (!f) return nvfi_fail(2, "%s: f must not be NULL", who);
    if (int rc = ml_mask_check(who, m)) return rc;
    if (int rc = ml_shape_check(who, R, f->n_samples, chunk_cap)) return rc;
    if ((labels != nullptr) == (soft != nullptr)) return nvfi_fail(2, "%s: exactly one of labels and soft must be given", who);
    if (kind != 0 && kind != 1) return nvfi_fail(2, "%s: kind=%d (0 l2, 1 ce)", who, kind);
    if (kind == 1 && !(eps > 0.f)) return nvfi_fail(2, "%s: eps=%g, the cross-entropy needs eps > 0", who, eps);
    if (loss_flags & ~NVFI_MASKLOSS_ADD_GW) return nvfi_fail(2, "%s: unknown loss_flags %d", who, loss_flags);
    if ((loss_flags & NVFI_MASKLOSS_ADD_GW) && !g_weights) return nvfi_fail(2, "%s: NVFI_MASKLOSS_ADD_GW without g_weights", who);
    if (!weights || !render_workspace) return nvfi_fail(2, "%s: weights and the render workspace must not be NULL", who);
    MlPlan P;
    plan_mask_loss(R, f->n_samples, chunk_cap, workspace, &P);
    if (int rc = ml_ws_check(who, P, workspace, workspace_bytes)) return rc;
    RenderPlan RP;     // the forward's, for reading: the masked list, its per-ray offsets, the device-side count, the warped positions
    if (int rc = render_plan_at(f, R, flags, t, const_cast<void*>(render_workspace), render_workspace_bytes, &RP)) return rc;
    if (ml_attrs()) return 1;
    const int64_t N = RP.N;
    MlArgs a; memset(&a, 0, sizeof(a));
    PackJobs jobs;
    ml_frags(m, P.frag, &a.W, &jobs);
    if (launch_pack(jobs, st)) return 1;
    a.K = m->mask_dim; a.S = f->n_samples; a.R = R; a.cap = N;
    a.count = RP.counters + 1; a.off_m = RP.off_m; a.list = RP.mlist; a.xw = RP.xw; a.weight = weights;
    a.hdr = P.hdr; a.lterm = P.lterm; a.vflag = P.vflag; a.gq = P.gq; a.pxw = P.pxw; a.ray = P.ray; a.maskv = P.maskv;
    a.labels = labels; a.soft = soft; a.kind = kind; a.eps = eps;
    a.grad_scale = grad_scale; a.grad_scale_dev = grad_scale_dev; a.add_gw = (loss_flags & NVFI_MASKLOSS_ADD_GW) ? 1 : 0;
    a.loss = loss; a.mask_map = mask_map; a.g_weights = g_weights;
    const dim3 gR((unsigned)((R + 3) / 4)), b256(256);
    hipLaunchKernelGGL(k_ml_fwd<false>, dim3((unsigned)((N + WG_SAMPLES - 1) / WG_SAMPLES)), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, a);
    LAUNCHCK();
    hipLaunchKernelGGL(k_ml_ray, gR, b256, 0, st, a);
    LAUNCHCK();
    hipLaunchKernelGGL(k_ml_mean, dim3(1), dim3(ML_MEAN_THREADS), 0, st, a);
    LAUNCHCK();
    if (g_weights && !a.add_gw)
        if (int rc = launch_zero(g_weights, N * (int64_t)sizeof(float), st)) return rc;
    hipLaunchKernelGGL(k_ml_grad, gR, b256, 0, st, a);
    LAUNCHCK();
    return 0;
}

extern "C" int nvfi_mask_loss_bwd(const nvfi_mask_desc* m, int64_t R, int S, int64_t first, int64_t chunk_cap, const nvfi_mask_grads* grads,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "nvfi_mask_loss_bwd";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = ml_mask_check(who, m)) return rc;
    if (int rc = ml_shape_check(who, R, S, chunk_cap)) return rc;
    const int64_t cap = R * (int64_t)S;
    if (first < 0 || first >= cap || first % chunk_cap) return nvfi_fail(2, "%s: first=%lld is not a multiple of chunk_cap=%lld inside the %lld entries of the call", who, (long long)first, (long long)chunk_cap, (long long)cap);
    if (!grads) return nvfi_fail(2, "%s: grads is NULL", who);
    MlPlan P;
    plan_mask_loss(R, S, chunk_cap, workspace, &P);
    if (int rc = ml_ws_check(who, P, workspace, workspace_bytes)) return rc;
    if (ml_attrs()) return 1;
    MlArgs a; memset(&a, 0, sizeof(a));
    ml_frags(nullptr, P.frag, &a.W, nullptr);          // packed by the forward
    a.K = m->mask_dim; a.S = S; a.R = R; a.cap = cap;
    a.hdr = P.hdr; a.gq = P.gq; a.pxw = P.pxw; a.ray = P.ray;
    a.first = first; a.chunk_cap = chunk_cap; a.ccount = P.ccount; a.relu = P.relu; a.stash_f = P.stash_f; a.stash_b = P.stash_b;
    const dim3 grid((unsigned)(chunk_cap / WG_SAMPLES)), block(WG_THREADS);
    hipLaunchKernelGGL(k_ml_fwd<true>, grid, block, ENGINE_LDS_BYTES, st, a);
    LAUNCHCK();
    hipLaunchKernelGGL(k_ml_adj, grid, block, ENGINE_LDS_BYTES, st, a);
    LAUNCHCK();
    // weight gradients: dW_l = g_z_l^T h_{l-1}, db_l = sum g_z_l - the jobs of nvfi_maskfield_bwd on the chunk's device count
    WgradJobs wj; wj.n = 0; ReduceJobs rj; rj.n = 0;
    const size_t fs = MK_F_ROWS * REGF, bs = MK_B_ROWS * REGF;
    for (int l = 0; l < 5; ++l) {
        if (!grads->W[l] && !grads->b[l]) continue;
        WgradJob& J = wj.j[wj.n];
        memset(&J, 0, sizeof(J));
        J.A = l == 4 ? P.stash_b : P.stash_b + (size_t)(16 + 64 * (3 - l)) * REGF; J.a_regs = l == 4 ? 16 : 64; J.a_tile_stride = bs;
        J.B = l == 0 ? P.stash_f : P.stash_f + (size_t)(16 + 64 * (l - 1)) * REGF; J.b_regs = l == 0 ? 16 : 64; J.b_tile_stride = fs;
        J.bmode = BM_RAW; J.count = P.ccount; J.cap_tiles = (int)P.tiles; J.nrep = 1;
        J.slabs = P.slabs + (size_t)wj.n * MK_NSLAB * MK_SLAB_FLOATS; J.nslab = MK_NSLAB;
        ReduceJob& Q = rj.j[rj.n++];
        memset(&Q, 0, sizeof(Q));
        Q.slabs = J.slabs; Q.nslab = MK_NSLAB; Q.MTA = J.a_regs / 16; Q.KTB = J.b_regs / 16; Q.gW = grads->W[l]; Q.gb = grads->b[l];
        Q.out = l < 4 ? 128 : m->mask_dim; Q.in = l == 0 ? 3 : 128; Q.row_kind = RK_NATURAL; Q.slot_kind = l == 0 ? SK_XYZ : SK_HIDDEN; Q.scale = 1.f;
        ++wj.n;
    }
    return launch_wgrad(wj, rj, st);
}
