// depthloss.hip - depth supervision (reference utils/evaluation_utils.py:8-17, compute_depth_loss(pred, gt)): each map is shifted by its median
// and scaled by its mean absolute deviation, the loss is the MSE of the two normalised maps.  Value and d(loss)/d(pred) in ONE launch of ONE
// workgroup, like k_mse (optim.hip): a training batch is 2 048 depths, and the torch form is two torch.median calls plus ~20 element-wise and
// reduce launches on a step that is a chain of dependent launches.
//   median   lower median (sorted element (n_c - 1) / 2, what torch.median returns) of the counted entries, by a radix select over
//            order-preserving 32-bit keys: 4 passes of 8 bits, both maps in the same pass.  Histograms live in LDS (4 copies per map, waves
//            w, w + 4, .. share one); a wave first folds the lanes that share the bin of its leading lanes into one add (depth maps have
//            plateaus: every ray that hits nothing has depth == far), the rest add singly.  Counts are integers: order cannot change them.
//   sums     two passes of fp64 sums (tie count, both deviations | loss, A, B, sum of signs) reduced wave -> workgroup in a fixed order (reduce.h), so two
//            calls on the same input give the same bits; per-entry arithmetic is fp64 too, the results are rounded to fp32 once.
//   gradient torch's full-tensor median spreads its gradient equally over all entries EQUAL to the median (float compare: -0.0 == +0.0):
//            e_j = [p_j == med] / c,  a_j = 2 (u_j - v_j) / n_c,  A = sum a_j,  B = sum a_j (p_j - med),  sg_j = sign(p_j - med)
//            dL/dp_j = a_j / (s + eps) - e_j A / (s + eps) - B / (s + eps)^2 (sg_j - e_j sum(sg)) / n_c
//   memory   n <= NVFI_DEPTH_LDS_MAX: both maps are read once and kept in LDS (2 x 4 n bytes, up to 128 KiB + 8.5 KiB of histograms and
//            partial sums); above, every pass streams them from global memory (a 640 000-entry frame is 5 MB: it stays in L2).
// No global atomics, no memset, no host synchronisation: the call can be captured in a hipGraph.
#include "reduce.h"

#define DL_THREADS 1024
#define DL_WAVES (DL_THREADS / 64)
#define DL_COPIES 4
#define DL_NSUM 4
#define DL_HEAD_BYTES (DL_WAVES * DL_NSUM * 8 + 2 * DL_COPIES * 256 * 4 + 8 * 4)      /* partial sums | histograms | select state */
#define DL_MAX_N (1 << 22)

__device__ __forceinline__ unsigned dl_key(float x) {                 // order-preserving: a < b (as floats) => key(a) < key(b); -0.0 sorts below +0.0
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dl_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool dl_counted(float g, int flags) { return !(flags & NVFI_DEPTH_SKIP_HOLES) || (g > 0.f && g < INFINITY); }

// every lane of the wave calls this (uniform control flow); `active` lanes add 1 to h[bin].  Two rounds fold all lanes that share the bin of the
// first still-active lane into one add of their count, what is left adds singly.
__device__ __forceinline__ void dl_hist_add(unsigned* h, unsigned bin, bool active, int lane) {
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const unsigned b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(active && bin == b0);
        if (lane == leader) atomicAdd(&h[b0], (unsigned)__popcll(same));
        if (bin == b0) active = false;
        m &= ~same;
    }
    if (active) atomicAdd(&h[bin], 1u);
}

// one whole wave: sums the copies of a 256-bin histogram (and clears them), finds the bin that holds sorted element st[1] among the entries
// counted in it, and appends the bin to the key prefix st[0].  first: st[2] = number of entries, st[1] = (n_c - 1) / 2 before the search.
__device__ __forceinline__ void dl_select(unsigned* hist, unsigned* st, int shift, bool first, int lane) {
    unsigned c[4], t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = 0;
#pragma unroll
        for (int q = 0; q < DL_COPIES; ++q) { c[j] += hist[q * 256 + 4 * lane + j]; hist[q * 256 + 4 * lane + j] = 0u; }
        t += c[j];
    }
    unsigned incl = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const unsigned total = __shfl(incl, 63);
    unsigned k = st[1];
    if (first) {
        k = total ? (total - 1u) / 2u : 0u;
        if (lane == 0) st[2] = total;
    }
    if (total == 0u) return;                          // nothing is counted: the caller leaves through its zero path
    const unsigned excl = incl - t;
    if (excl <= k && k < incl) {                      // exactly one lane: the bins of the lanes in front hold excl entries
        unsigned kk = k - excl;
        int j = 0;
        while (j < 3 && kk >= c[j]) { kk -= c[j]; ++j; }
        st[0] |= (unsigned)(4 * lane + j) << shift;
        st[1] = kk;
    }
}

template <bool IN_LDS>
__global__ __launch_bounds__(DL_THREADS) void k_depth_loss(int64_t n, const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const int64_t* __restrict__ gt_index, int flags, float grad_scale,
                                                           float* __restrict__ loss, float* __restrict__ g_pred, int64_t* __restrict__ n_counted) {
    extern __shared__ __align__(16) unsigned char dl_smem[];
    double* part = reinterpret_cast<double*>(dl_smem);
    unsigned* hist = reinterpret_cast<unsigned*>(dl_smem + DL_WAVES * DL_NSUM * 8);       // [map][copy][256]
    unsigned* st = hist + 2 * DL_COPIES * 256;                                             // [map][4]: key prefix, rank, n_c
    float* lp = reinterpret_cast<float*>(dl_smem + DL_HEAD_BYTES);                         // IN_LDS: pred (n) | target (n)
    float* lg = lp + (IN_LDS ? n : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < 2 * DL_COPIES * 256; i += DL_THREADS) hist[i] = 0u;
    if (tid < 8) st[tid] = 0u;
    __syncthreads();

    unsigned* hp = hist + (wave & (DL_COPIES - 1)) * 256;
    unsigned* hg = hp + DL_COPIES * 256;
    // ---- both medians: 4 x 8 bits, most significant first
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
        const unsigned pre_p = st[0], pre_g = st[4];
        for (int64_t base = 0; base < n; base += DL_THREADS) {          // wave-uniform trip count: dl_hist_add needs the whole wave
            const int64_t i = base + tid;
            const bool in = i < n;
            float p = 0.f, g = 0.f;
            if (in) {
                if (IN_LDS && pass) { p = lp[i]; g = lg[i]; }
                else {
                    p = pred[i];
                    g = gt[gt_index ? gt_index[i] : i];
                    if (IN_LDS) { lp[i] = p; lg[i] = g; }
                }
            }
            const bool cnt = in && dl_counted(g, flags);
            const unsigned kp = dl_key(p), kg = dl_key(g);
            dl_hist_add(hp, (kp >> shift) & 255u, cnt && (kp & himask) == pre_p, lane);
            dl_hist_add(hg, (kg >> shift) & 255u, cnt && (kg & himask) == pre_g, lane);
        }
        __syncthreads();
        if (wave < 2) dl_select(hist + wave * DL_COPIES * 256, st + 4 * wave, shift, pass == 0, lane);
        __syncthreads();
        if (st[2] == 0u) {                                                // all holes: loss 0, gradient 0, count 0
            for (int64_t i = tid; i < n; i += DL_THREADS) g_pred[i] = 0.f;
            if (tid == 0) { *loss = 0.f; if (n_counted) *n_counted = 0; }
            return;
        }
    }
    const unsigned nc = st[2];
    const float med_p = dl_unkey(st[0]), med_g = dl_unkey(st[4]);
    const double inv_n = 1.0 / (double)nc;

    // ---- tie count and both mean absolute deviations
    double v[DL_NSUM] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = tid; i < n; i += DL_THREADS) {
        const float p = IN_LDS ? lp[i] : pred[i];
        const float g = IN_LDS ? lg[i] : gt[gt_index ? gt_index[i] : i];
        if (!dl_counted(g, flags)) continue;
        v[0] += p == med_p ? 1.0 : 0.0;
        v[1] += fabs((double)p - (double)med_p);
        v[2] += fabs((double)g - (double)med_g);
    }
    block_sum_ordered<DL_WAVES, DL_NSUM>(v, part, lane, wave);
    const double ties = v[0];
    const double inv_p = 1.0 / (v[1] * inv_n + 1e-6), inv_g = 1.0 / (v[2] * inv_n + 1e-6);

    // ---- loss, A, B, sum of signs (d = u - v; a = 2 d / n_c)
    v[0] = v[1] = v[2] = v[3] = 0.0;
    for (int64_t i = tid; i < n; i += DL_THREADS) {
        const float p = IN_LDS ? lp[i] : pred[i];
        const float g = IN_LDS ? lg[i] : gt[gt_index ? gt_index[i] : i];
        if (!dl_counted(g, flags)) continue;
        const double dp = (double)p - (double)med_p;
        const double d = dp * inv_p - ((double)g - (double)med_g) * inv_g;
        v[0] += d * d;
        v[1] += d;
        v[2] += d * dp;
        v[3] += dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0);
    }
    block_sum_ordered<DL_WAVES, DL_NSUM>(v, part, lane, wave);
    const double A = 2.0 * inv_n * v[1], B = 2.0 * inv_n * v[2], sum_sg = v[3];
    if (tid == 0) {
        *loss = (float)(v[0] * inv_n);
        if (n_counted) *n_counted = (int64_t)nc;
    }

    // ---- gradient
    const double e_tie = 1.0 / ties, cB = B * inv_p * inv_p * inv_n, gs = (double)grad_scale;
    for (int64_t i = tid; i < n; i += DL_THREADS) {
        const float p = IN_LDS ? lp[i] : pred[i];
        const float g = IN_LDS ? lg[i] : gt[gt_index ? gt_index[i] : i];
        if (!dl_counted(g, flags)) { g_pred[i] = 0.f; continue; }
        const double dp = (double)p - (double)med_p;
        const double d = dp * inv_p - ((double)g - (double)med_g) * inv_g;
        const double e = p == med_p ? e_tie : 0.0;
        const double sg = dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0);
        g_pred[i] = (float)(gs * ((2.0 * inv_n * d - e * A) * inv_p - cB * (sg - e * sum_sg)));
    }
}

extern "C" int nvfi_depth_loss(int64_t n, const float* pred, const float* gt, const int64_t* gt_index, int flags, float grad_scale,
                               float* loss, float* g_pred, int64_t* n_counted, void* stream) {
    if (n <= 0) return nvfi_fail(2, "nvfi_depth_loss: n must be positive");
    if (n > DL_MAX_N) return nvfi_fail(2, "nvfi_depth_loss: one-workgroup kernel, n <= 4194304");
    if (!pred || !gt || !loss || !g_pred) return nvfi_fail(2, "nvfi_depth_loss: pred, gt, loss and g_pred must not be NULL");
    if (flags & ~NVFI_DEPTH_SKIP_HOLES) return nvfi_fail(2, "nvfi_depth_loss: unknown flags %d", flags);
    hipStream_t st = (hipStream_t)stream;
    if (n <= NVFI_DEPTH_LDS_MAX) {
        static DeviceOnce once;
        if (once.lds(DL_HEAD_BYTES + 8 * NVFI_DEPTH_LDS_MAX, k_depth_loss<true>)) return 1;
        hipLaunchKernelGGL(k_depth_loss<true>, dim3(1), dim3(DL_THREADS), (size_t)(DL_HEAD_BYTES + 8 * n), st, n, pred, gt, gt_index, flags, grad_scale,
                           loss, g_pred, n_counted);
    } else {
        hipLaunchKernelGGL(k_depth_loss<false>, dim3(1), dim3(DL_THREADS), (size_t)DL_HEAD_BYTES, st, n, pred, gt, gt_index, flags, grad_scale,
                           loss, g_pred, n_counted);
    }
    LAUNCHCK();
    return 0;
}
