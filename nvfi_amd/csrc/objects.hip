// objects.hip - per-object layers and the object-selected render of a MaskField decomposition (nvfi_render_objects, and the hot path of
// nvfi_render_fwd_select; the reference has no counterpart: its mask branch stops at the soft label map, tensorf_keyframe.py:749-753).
//
// Both are inference branches of the render, built like the mask and flow branches (render_blocks.hip: nvfi_render_mask, flow.hip):
//   k_obj_final     behind nvfi_render_fwd + nvfi_render_mask on the workspace they filled: one wave per ray walks the ray's appearance-masked
//                   entries ONCE (off_m, mlist) and accumulates, per object k, sum w m_k, sum w m_k c (3) and sum w m_k z - all 5 K sums of the
//                   ray from that one pass, in list order, without atomics.  The lane layout (entry parity x 32 channels) and the order of the
//                   additions are k_mask_final's, so obj_acc carries the bits of mask_map.
//   k_select_fwd    between the density and the weights kernels of nvfi_render_fwd_select: the MaskField (3 -> 128 x 4 ReLU -> K, softmax) over the
//                   V VALID samples of the chunk at their warped keyframe positions - k_mask_fwd's fp32 MFMA sample-tile pipeline (engine.h) over
//                   the valid list instead of the masked one - whose epilogue reduces the softmax against `select` in registers and writes ONE
//                   float per sample, s(x) = sum_k select_k softmax_k; k_weights_fill<SEL> / k_weights_fwd<SEL> multiply the density by it.
//                   No (V, 32) array exists.  V (3 128 + 3 128^2 + 128 K) multiply-adds per call.
// fp32 MFMA only (engine.h, like k_mask_fwd): no 16-bit matrix instruction is issued here, so the unit needs no packed-fp32 fence.
#include <string.h>
#include "common.h"
#include "render.h"

struct SelArgs {
    const float* f[5]; const float* b[5]; int mask_dim;
    const int* count; const int* list; const float4* xw;
    const float* select; float* sel;
};

__global__ __launch_bounds__(WG_THREADS, 2) void k_select_fwd(SelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int count = *a.count;
    if ((int)(blockIdx.x * WG_SAMPLES) >= count) return;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = i < count;
    const int n = active ? a.list[i] : 0;
    const float4 q = active ? a.xw[n] : zero4();
    float xa[64], xb[64];
    xb[0] = h ? q.y : q.x; xb[1] = h ? 0.f : q.z;
    __syncthreads();
    stage_frag(lds_w, lds_b, a.f[0], 4 * 2 * 64, a.b[0], 128);
    __syncthreads();
    layer_tiles<4, 2>(lds_w, lds_b, true, lane, h, xb, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xa[16 * m + r] = fmaxf(acc[r], 0.f);
    });
    __syncthreads();
    stage_frag(lds_w, lds_b, a.f[1], 4 * 64 * 64, a.b[1], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xa, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xb[16 * m + r] = fmaxf(acc[r], 0.f);
    });
    __syncthreads();
    stage_frag(lds_w, lds_b, a.f[2], 4 * 64 * 64, a.b[2], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xb, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xa[16 * m + r] = fmaxf(acc[r], 0.f);
    });
    __syncthreads();
    stage_frag(lds_w, lds_b, a.f[3], 4 * 64 * 64, a.b[3], 128);
    __syncthreads();
    layer_tiles<4, 64>(lds_w, lds_b, true, lane, h, xa, [&](int m, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xb[16 * m + r] = fmaxf(acc[r], 0.f);
    });
    __syncthreads();
    stage_frag(lds_w, lds_b, a.f[4], 1 * 64 * 64, a.b[4], 32);
    __syncthreads();
    float o[16];
    layer_tiles<1, 64>(lds_w, lds_b, true, lane, h, xb, [&](int, const f32x16& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = acc[r];
    });
    // softmax over the mask_dim logits of the sample, reduced against select in place: rows (r&3)+8(r>>2)+4h live in this lane, the rest in lane^32
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int row = (r & 3) + 8 * (r >> 2) + 4 * h; if (row < a.mask_dim) mx = fmaxf(mx, o[r]); }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f, num = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < a.mask_dim) { const float e = expf(o[r] - mx); sum += e; num += a.select[row] * e; }
    }
    sum += __shfl_xor(sum, 32); num += __shfl_xor(num, 32);
    if (active && h == 0) a.sel[n] = num / sum;
}

static int mask_desc_check(const nvfi_mask_desc* m) {
    if (m->n_layer != 4 || m->n_dim != 128 || m->mask_dim < 1 || m->mask_dim > 32)
        return nvfi_fail(2, "mask field must be 3->128x4->mask_dim<=32 (train_segm.py:97-102); got n_layer=%d n_dim=%d mask_dim=%d", m->n_layer, m->n_dim, m->mask_dim);
    for (int l = 0; l < 5; ++l) if (!m->W[l] || !m->b[l]) return nvfi_fail(2, "mask field layer %d has no weight/bias pointer", l);
    return 0;
}

int launch_select(const nvfi_mask_desc* m, const float* select, const int* count_v, const int* vlist, const float4* xw, float* sel, float* frag,
                  int64_t N, hipStream_t st) {
    if (mask_desc_check(m)) return 2;
    if (!sel || !frag) return nvfi_fail(2, "nvfi_render_fwd_select needs a workspace planned with NVFI_WANT_SELECT in flags");
    static DeviceOnce once;
    if (once.lds(ENGINE_LDS_BYTES, k_select_fwd)) return 1;
    // the fragments of nvfi_render_mask (same layout), packed once per call
    PackJobs jobs; jobs.n = 0;
    SelArgs a; memset(&a, 0, sizeof(a));
    float* p = frag;
    for (int l = 0; l < 5; ++l) {
        PackJob& J = jobs.j[jobs.n++];
        memset(&J, 0, sizeof(J));
        const int MT = l < 4 ? 4 : 1, NS = l == 0 ? 2 : 64;
        J.W = m->W[l]; J.b = m->b[l]; J.frag = p; p += MT * NS * 64; J.bfrag = p; p += 128;
        J.out = l < 4 ? 128 : m->mask_dim; J.in = l == 0 ? 3 : 128; J.MT = MT; J.NS = NS;
        J.row_kind = RK_NATURAL; J.slot_kind = l == 0 ? SK_XYZ : SK_HIDDEN; J.transposed = 0; J.x4 = 0;
        a.f[l] = J.frag; a.b[l] = J.bfrag;
    }
    if (launch_pack(jobs, st)) return 1;
    a.mask_dim = m->mask_dim; a.count = count_v; a.list = vlist; a.xw = xw; a.select = select; a.sel = sel;
    const unsigned wgs = (unsigned)((N + WG_SAMPLES - 1) / WG_SAMPLES);
    hipLaunchKernelGGL(k_select_fwd, dim3(wgs), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, a);
    LAUNCHCK();
    return 0;
}

struct ObjArgs {
    int64_t R; int K;
    const int* off_m; const int* list; const float* weight; const float4* xw; const float4* rgbs; const float* maskv;
    float* obj_rgb; float* obj_acc; float* obj_depth;
};

// one wave per ray; lane = (entry parity e, channel k of 32) as in k_mask_final: two entries per pass, every lane adds its own entries in list
// order, then the two parities are added - the same bits every call, and for obj_acc the bits of mask_map
__global__ __launch_bounds__(256) void k_obj_final(ObjArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
    const int k = lane & 31, e0 = lane >> 5;
    float s = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dz = 0.f;
    for (int i = b0 + e0; i < b1; i += 2) {
        const int n = a.list[i];
        const float wm = a.weight[n] * (k < a.K ? a.maskv[(size_t)i * 32 + k] : 0.f);
        const float4 c = a.rgbs[i];
        const float z = a.xw[n].w;
        s += wm;
        c0 += wm * c.x; c1 += wm * c.y; c2 += wm * c.z;
        dz += wm * z;
    }
    s += __shfl_xor(s, 32); c0 += __shfl_xor(c0, 32); c1 += __shfl_xor(c1, 32); c2 += __shfl_xor(c2, 32); dz += __shfl_xor(dz, 32);
    if (lane < a.K) {
        const int64_t o = r * a.K + lane;
        if (a.obj_acc) a.obj_acc[o] = s;
        if (a.obj_rgb) { a.obj_rgb[3 * o] = c0; a.obj_rgb[3 * o + 1] = c1; a.obj_rgb[3 * o + 2] = c2; }
        if (a.obj_depth) a.obj_depth[o] = dz;
    }
}

extern "C" int nvfi_render_objects(const nvfi_field_desc* f, const nvfi_mask_desc* m, int64_t R, float t, int flags, const float* weights,
                                   float* obj_rgb, float* obj_acc, float* obj_depth, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (mask_desc_check(m)) return 2;
    if (R <= 0) return 0;
    if (flags & NVFI_TRAIN) return nvfi_fail(2, "nvfi_render_objects is an inference branch: NVFI_TRAIN renders have none");
    if (!(flags & NVFI_WANT_MASK)) return nvfi_fail(2, "nvfi_render_objects needs a workspace planned with NVFI_WANT_MASK in flags");
    RenderPlan P;      // what nvfi_render_fwd + nvfi_render_mask filled
    const int rc = render_plan_at(f, R, flags, t, workspace, workspace_bytes, &P);
    if (rc == 4)
        return nvfi_fail(2, "workspace of %lld bytes, the plan of these flags needs %lld: nvfi_render_objects needs the workspace of the render call", (long long)workspace_bytes, (long long)P.total);
    if (rc) return rc;
    if (!P.maskv) return nvfi_fail(2, "nvfi_render_objects needs a workspace planned with NVFI_WANT_MASK in flags");
    if (!obj_rgb && !obj_acc && !obj_depth) return 0;
    ObjArgs a; memset(&a, 0, sizeof(a));
    a.R = R; a.K = m->mask_dim; a.off_m = P.off_m; a.list = P.mlist; a.weight = weights; a.xw = P.xw; a.rgbs = P.rgbs; a.maskv = P.maskv;
    a.obj_rgb = obj_rgb; a.obj_acc = obj_acc; a.obj_depth = obj_depth;
    hipLaunchKernelGGL(k_obj_final, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, a);
    LAUNCHCK();
    return 0;
}
