// metrics.hip - the numbers of the reference's two evaluation scripts on the GPU, next to the frames they score: nvfi_ssim (utils/metrics.py:32-99)
// and nvfi_segm_confusion (the per-frame statistics that every quantity of utils/metric_segm.py is a function of) of include/nvfi_hip.h.
//
//   nvfi_ssim            k_met_clear       tickets
//                        k_ssim_range      (derived dynamic range only) min / max of pred per image in two stages, last workgroup per image
//                        k_ssim            one workgroup per 32 x 16 output tile and channel: the tile + a 10-pixel halo of both images in LDS,
//                                          horizontal pass -> five moment planes in LDS, vertical pass -> SSIM and cs per output pixel, wave
//                                          reduction, ONE partial pair per workgroup; the last workgroup of an image sums its partials
//   nvfi_segm_confusion  k_met_clear       tickets, bad-label counters, counts
//                        k_segm_confusion  per pixel: argmax of the K mask values (lowest index on ties), (label, argmax) pairs aggregated per wave
//                                          before the workgroup's LDS histogram, integer atomics into counts[G][K]; the confidence sums go through
//                                          per-workgroup slots, the last workgroup of a frame sums them
// Arithmetic: the windowed moments are second moments whose differences (E[x^2] - mu^2) cancel; both passes therefore accumulate in fp64 (fp32
// products are exact there), and the SSIM formula is evaluated in fp64.  The per-pixel work is ~130 fp64 FMAs, a few tens of microseconds per
// 800 x 800 x 3 frame: the kernel stays bound by its launches.
// House rules and the in-launch hand-off (publish, last_arrival, read_published): reduce.h - the results repeat bit for bit.
#include <limits.h>
#include <string.h>
#include "reduce.h"

#define MET_WGS 256              // workgroups per frame of the grid-stride kernels (= partials per value)
#define MET_MAX_K 32
#define MET_MAX_G 32
#define MET_MAX_B 65535
#define SSIM_W 11
#define SSIM_TW 32               // output tile
#define SSIM_TH 16
#define SSIM_IW (SSIM_TW + SSIM_W - 1)
#define SSIM_IH (SSIM_TH + SSIM_W - 1)

// sum of n partials at p[i * stride] by the whole workgroup (256 threads) in a fixed order: thread t takes i = t, t + 256, ...; wave tree; waves 0..3.
// Not reduce.h's block_sum_ordered: the four wave sums are added PAIRWISE (as in the publishes of k_ssim and k_segm_confusion) - the sequential
// order gives other bits
__device__ __forceinline__ double met_block_sum(const double* p, int64_t n, int64_t stride, double* red4) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += read_published(p + i * stride);
    s = wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

__global__ __launch_bounds__(256) void k_met_clear(int* a, int64_t na, int* b, int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = 0;
    else if (i - na < nb) b[i - na] = 0;
}

// ---------------------------------------------------------------- SSIM
struct SsimArgs {
    int B, C, H, W;
    const float* pred; const float* gt;
    int64_t ps[4], gs[4];            // element strides of (image, channel, row, column)
    float win[SSIM_W];
    int range_mode;                  // 0: L given; 1: derived from all images of the call; 2: derived per image
    float L;
    double* out;                     // (B, 2): mean SSIM, mean cs
    double* part; float* rpart; float* range; int* tickets;
    int tiles_x, tiles_y;
};

// min / max of pred per image: grid (MET_WGS, B)
__global__ __launch_bounds__(256) void k_ssim_range(SsimArgs a) {
    __shared__ float red[4][2];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t hw = (int64_t)a.H * a.W, n = hw * a.C;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / hw);
        const int64_t r = i - c * hw;
        const int y = (int)(r / a.W), x = (int)(r - (int64_t)y * a.W);
        const float v = a.pred[b * a.ps[0] + c * a.ps[1] + y * a.ps[2] + x * a.ps[3]];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if (lane == 0) { red[wv][0] = lo; red[wv][1] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        publish(a.rpart + ((int64_t)b * gridDim.x + blockIdx.x) * 2, fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0])));
        publish(a.rpart + ((int64_t)b * gridDim.x + blockIdx.x) * 2 + 1, fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1])));
    }
    if (!last_arrival(a.tickets + a.B + b, (int)gridDim.x)) return;
    if (wv == 0) {
        lo = INFINITY; hi = -INFINITY;
        for (int w = lane; w < (int)gridDim.x; w += 64) {
            lo = fminf(lo, read_published(a.rpart + ((int64_t)b * gridDim.x + w) * 2));
            hi = fmaxf(hi, read_published(a.rpart + ((int64_t)b * gridDim.x + w) * 2 + 1));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
        if (lane == 0) { a.range[2 * b] = lo; a.range[2 * b + 1] = hi; }
    }
}

// grid (tiles_x * tiles_y, C, B)
__global__ __launch_bounds__(256) void k_ssim(SsimArgs a) {
    __shared__ float sp[SSIM_IH][SSIM_IW + 1], sg[SSIM_IH][SSIM_IW + 1];
    __shared__ double mom[5][SSIM_IH][SSIM_TW];
    __shared__ double red[4][2];
    __shared__ double red4[4];
    __shared__ float sL;
    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = tx * SSIM_TW, y0 = ty * SSIM_TH;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* P = a.pred + b * a.ps[0] + c * a.ps[1];
    const float* G = a.gt + b * a.gs[0] + c * a.gs[1];
    for (int i = threadIdx.x; i < SSIM_IH * SSIM_IW; i += 256) {
        const int r = i / SSIM_IW, q = i - r * SSIM_IW;
        const int y = y0 + r, x = x0 + q;
        const bool in = y < a.H && x < a.W;          // beyond the image: zeros, which reach invalid outputs only
        sp[r][q] = in ? P[y * a.ps[2] + x * a.ps[3]] : 0.f;
        sg[r][q] = in ? G[y * a.gs[2] + x * a.gs[3]] : 0.f;
    }
    if (wv == 0 && a.range_mode != 0) {              // the dynamic range by the reference's rule (metrics.py:57-66), from device memory
        float lo = INFINITY, hi = -INFINITY;
        if (a.range_mode == 2) { lo = a.range[2 * b]; hi = a.range[2 * b + 1]; }
        else {
            for (int i = lane; i < a.B; i += 64) { lo = fminf(lo, a.range[2 * i]); hi = fmaxf(hi, a.range[2 * i + 1]); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
        }
        if (lane == 0) sL = (hi > 128.f ? 255.f : 1.f) - (lo < -0.5f ? -1.f : 0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SSIM_IH * SSIM_TW; i += 256) {
        const int r = i / SSIM_TW, x = i - r * SSIM_TW;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SSIM_W; ++k) {
            const double w = (double)a.win[k], p = (double)sp[r][x + k], g = (double)sg[r][x + k];
            m[0] += w * p; m[1] += w * g; m[2] += w * (p * p); m[3] += w * (g * g); m[4] += w * (p * g);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) mom[j][r][x] = m[j];
    }
    __syncthreads();
    const double L = a.range_mode != 0 ? (double)sL : (double)a.L;
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    double acc_s = 0.0, acc_c = 0.0;
    for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += 256) {
        const int y = i / SSIM_TW, x = i - y * SSIM_TW;
        if (y0 + y >= a.H - (SSIM_W - 1) || x0 + x >= a.W - (SSIM_W - 1)) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SSIM_W; ++k) {
            const double w = (double)a.win[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += w * mom[j][y + k][x];
        }
        const double mu11 = m[0] * m[0], mu22 = m[1] * m[1], mu12 = m[0] * m[1];
        const double v1 = 2.0 * (m[4] - mu12) + C2, v2 = (m[2] - mu11) + (m[3] - mu22) + C2;
        acc_c += v1 / v2;
        acc_s += ((2.0 * mu12 + C1) * v1) / ((mu11 + mu22 + C1) * v2);
    }
    acc_s = wave_sum(acc_s); acc_c = wave_sum(acc_c);
    if (lane == 0) { red[wv][0] = acc_s; red[wv][1] = acc_c; }
    __syncthreads();
    const int64_t per_image = (int64_t)a.C * gridDim.x;
    double* part = a.part + ((int64_t)b * per_image + (int64_t)c * gridDim.x + tile) * 2;
    if (threadIdx.x < 2) publish(part + threadIdx.x, (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
    if (!last_arrival(a.tickets + b, (int)per_image)) return;
    const double cnt = (double)a.C * (double)(a.H - (SSIM_W - 1)) * (double)(a.W - (SSIM_W - 1));
    const double* base = a.part + (int64_t)b * per_image * 2;
    const double s = met_block_sum(base, per_image, 2, red4);
    const double cs = met_block_sum(base + 1, per_image, 2, red4);
    if (threadIdx.x == 0) { a.out[2 * b] = s / cnt; a.out[2 * b + 1] = cs / cnt; }
}

// ---------------------------------------------------------------- segmentation confusion
struct ConfArgs {
    int B, K, G; int64_t N; bool vec;
    const float* mask; const int32_t* label;
    unsigned long long* counts;      // (B, G, K)
    double* conf_sum;                // (B, K)
    int32_t* pred;                   // (B, N) or NULL
    int32_t* bad;                    // (B): number of labels outside [0, G) - such a pixel is counted nowhere
    double* part; int* tickets; int* badws;
};

// grid (MET_WGS or fewer, B)
__global__ __launch_bounds__(256) void k_segm_confusion(ConfArgs a) {
    __shared__ int hist[MET_MAX_G * MET_MAX_K];
    __shared__ double wconf[4][MET_MAX_K];        // per wave: only its own lanes add to its row, in program order
    __shared__ int sbad;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cells = a.G * a.K;
    for (int i = threadIdx.x; i < cells; i += 256) hist[i] = 0;
    if (threadIdx.x < 4 * MET_MAX_K) wconf[threadIdx.x / MET_MAX_K][threadIdx.x % MET_MAX_K] = 0.0;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    const float* M = a.mask + (int64_t)b * a.N * a.K;
    const int32_t* Lb = a.label + (int64_t)b * a.N;
    int nbad = 0;
    for (int64_t n0 = (int64_t)blockIdx.x * 256; n0 < a.N; n0 += (int64_t)gridDim.x * 256) {
        const int64_t n = n0 + threadIdx.x;
        int pair = -1;
        double conf = 0.0;
        if (n < a.N) {
            const float* row = M + n * a.K;
            float best = -INFINITY; int k = 0;               // strict >: the lowest index wins a tie (numpy's argmax); NaN is outside the contract
            if (a.vec) {
#pragma unroll
                for (int q4 = 0; q4 < MET_MAX_K / 4; ++q4) {
                    if (4 * q4 >= a.K) continue;
                    const float4 v = ld4(row + 4 * q4);
                    if (v.x > best) { best = v.x; k = 4 * q4; }
                    if (v.y > best) { best = v.y; k = 4 * q4 + 1; }
                    if (v.z > best) { best = v.z; k = 4 * q4 + 2; }
                    if (v.w > best) { best = v.w; k = 4 * q4 + 3; }
                }
            } else {
                for (int c = 0; c < a.K; ++c) { const float v = row[c]; if (v > best) { best = v; k = c; } }
            }
            if (best == -INFINITY) best = row[0];            // a row of -inf: index 0, as numpy
            if (a.pred) a.pred[(int64_t)b * a.N + n] = k;
            const int g = Lb[n];
            if (g < 0 || g >= a.G) ++nbad;
            else { pair = g * a.K + k; conf = (double)best; }
        }
        // labels of a frame are spatially coherent: the wave's pixels share a handful of (label, argmax) pairs - one LDS atomic and one wave sum
        // of the confidences per distinct pair (fixed lane order, pairs in the order of their first lane: nothing depends on timing)
        unsigned long long todo = __ballot(pair >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lp = __shfl(pair, leader);
            const unsigned long long same = __ballot(pair == lp);
            const double cs = wave_sum(pair == lp ? conf : 0.0);
            if (lane == leader) { atomicAdd(&hist[lp], __popcll(same)); wconf[wv][lp % a.K] += cs; }
            todo &= ~same;
        }
    }
    if (nbad) atomicAdd(&sbad, nbad);
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256)
        if (hist[i]) atomicAdd(a.counts + (int64_t)b * cells + i, (unsigned long long)hist[i]);
    if (threadIdx.x == 0 && sbad) atomicAdd(a.badws + b, sbad);
    double* part = a.part + ((int64_t)b * gridDim.x + blockIdx.x) * MET_MAX_K;
    if ((int)threadIdx.x < a.K) { const int c = threadIdx.x; publish(part + c, (wconf[0][c] + wconf[1][c]) + (wconf[2][c] + wconf[3][c])); }
    if (!last_arrival(a.tickets + b, (int)gridDim.x)) return;
    if ((int)threadIdx.x < a.K) {
        const int c = threadIdx.x;
        double s = 0.0;
        for (int w = 0; w < (int)gridDim.x; ++w) s += read_published(a.part + ((int64_t)b * gridDim.x + w) * MET_MAX_K + c);
        a.conf_sum[(int64_t)b * a.K + c] = s;
    }
    if (threadIdx.x == 0) a.bad[b] = __hip_atomic_load(a.badws + b, RED_RLX);
}

// ---------------------------------------------------------------- host
struct MetPlan { int* tickets; int64_t n_int; double* part; float* rpart; float* range; int64_t total; };
static int64_t ssim_tiles(int H, int W, int* tx, int* ty) {
    *tx = (W - (SSIM_W - 1) + SSIM_TW - 1) / SSIM_TW; *ty = (H - (SSIM_W - 1) + SSIM_TH - 1) / SSIM_TH;
    return (int64_t)*tx * *ty;
}
// kind 0: nvfi_ssim(B, C, H, W); kind 1: nvfi_segm_confusion(B, N = H * W ignored here, K = C)
static void met_plan(int kind, int64_t B, int C, int H, int W, void* ws, MetPlan* P) {
    Bump Bm{(char*)ws, 0, 0};
    P->n_int = 2 * B;                                 // ssim: per-image tickets of k_ssim, of k_ssim_range; confusion: tickets, bad-label counters
    P->tickets = Bm.take<int>(P->n_int);
    if (kind == 0) {
        int tx, ty;
        P->part = Bm.take<double>(2 * B * C * ssim_tiles(H, W, &tx, &ty));
        P->rpart = Bm.take<float>(2 * B * MET_WGS);
        P->range = Bm.take<float>(2 * B);
    } else {
        P->part = Bm.take<double>(B * MET_WGS * MET_MAX_K);
        P->rpart = nullptr; P->range = nullptr;
    }
    P->total = align_up(Bm.off, 256);
}
static int ssim_sizes_ok(int64_t B, int C, int H, int W) {
    if (B < 1 || B > MET_MAX_B) return nvfi_fail(2, "nvfi_ssim: %lld images (1..%d are supported)", (long long)B, MET_MAX_B);
    if (C < 1 || C > 4) return nvfi_fail(2, "nvfi_ssim: %d channels (1..4 are supported)", C);
    if (H < SSIM_W || W < SSIM_W || H > 32768 || W > 32768) return nvfi_fail(2, "nvfi_ssim: %d x %d images (11 x 11 .. 32768 x 32768: the window has no padding)", H, W);
    return 0;
}
static int conf_sizes_ok(int64_t B, int64_t N, int K, int G) {
    if (B < 1 || B > MET_MAX_B) return nvfi_fail(2, "nvfi_segm_confusion: %lld frames (1..%d are supported)", (long long)B, MET_MAX_B);
    if (N < 1 || N > (1ll << 30)) return nvfi_fail(2, "nvfi_segm_confusion: N = %lld pixels is outside 1..2^30", (long long)N);
    if (K < 1 || K > MET_MAX_K) return nvfi_fail(2, "nvfi_segm_confusion: %d predicted classes (1..%d are supported)", K, MET_MAX_K);
    if (G < 1 || G > MET_MAX_G) return nvfi_fail(2, "nvfi_segm_confusion: %d ground-truth labels (1..%d are supported)", G, MET_MAX_G);
    return 0;
}
extern "C" int nvfi_metrics_workspace_bytes(int kind, int64_t B, int C, int H, int W, int64_t* bytes) {
    if (kind != 0 && kind != 1) return nvfi_fail(2, "nvfi_metrics_workspace_bytes: kind %d (0: nvfi_ssim, 1: nvfi_segm_confusion)", kind);
    if (kind == 0 ? ssim_sizes_ok(B, C, H, W) : conf_sizes_ok(B, 1, C, 1)) return 2;
    MetPlan P;
    met_plan(kind, B, C, H, W, nullptr, &P);
    *bytes = P.total;
    return 0;
}

static int met_clear(int* a, int64_t na, int* b, int64_t nb, hipStream_t st) {
    hipLaunchKernelGGL(k_met_clear, dim3((unsigned)((na + nb + 255) / 256)), dim3(256), 0, st, a, na, b, nb);
    LAUNCHCK();
    return 0;
}

extern "C" int nvfi_ssim(int64_t B, int C, int H, int W, const float* pred, const int64_t* pred_strides4, const float* gt, const int64_t* gt_strides4,
                         const float* window11, float L, int range_mode, double* out_b2, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (ssim_sizes_ok(B, C, H, W)) return 2;
    if (!pred || !gt || !pred_strides4 || !gt_strides4 || !window11 || !out_b2) return nvfi_fail(2, "nvfi_ssim: NULL argument");
    if (range_mode < 0 || range_mode > 2) return nvfi_fail(2, "nvfi_ssim: range_mode %d (0 given, 1 derived over the call, 2 derived per image)", range_mode);
    if (range_mode == 0 && !(L > 0.f)) return nvfi_fail(2, "nvfi_ssim: dynamic range L = %g", (double)L);
    for (int i = 0; i < 4; ++i)
        if (pred_strides4[i] < 0 || gt_strides4[i] < 0) return nvfi_fail(2, "nvfi_ssim: negative strides are not supported");
    MetPlan P;
    met_plan(0, B, C, H, W, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)P.total);
    SsimArgs a; memset(&a, 0, sizeof(a));
    a.B = (int)B; a.C = C; a.H = H; a.W = W; a.pred = pred; a.gt = gt;
    for (int i = 0; i < 4; ++i) { a.ps[i] = pred_strides4[i]; a.gs[i] = gt_strides4[i]; }
    for (int i = 0; i < SSIM_W; ++i) a.win[i] = window11[i];
    a.range_mode = range_mode; a.L = L; a.out = out_b2;
    a.part = P.part; a.rpart = P.rpart; a.range = P.range; a.tickets = P.tickets;
    const int64_t tiles = ssim_tiles(H, W, &a.tiles_x, &a.tiles_y);
    if (tiles * C > INT_MAX / 4) return nvfi_fail(2, "nvfi_ssim: too many tiles");
    if (met_clear(P.tickets, P.n_int, nullptr, 0, st)) return 1;
    if (range_mode != 0) {
        const int64_t n = (int64_t)C * H * W;
        const unsigned wgs = (unsigned)((n + 255) / 256 < MET_WGS ? (n + 255) / 256 : MET_WGS);
        hipLaunchKernelGGL(k_ssim_range, dim3(wgs, (unsigned)B), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)tiles, (unsigned)C, (unsigned)B), dim3(256), 0, st, a);
    LAUNCHCK();
    return 0;
}

extern "C" int nvfi_segm_confusion(int64_t B, int64_t N, int K, int G, const float* mask, const int32_t* labels, int64_t* counts, double* conf_sum,
                                   int32_t* pred_label, int32_t* bad_labels, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (conf_sizes_ok(B, N, K, G)) return 2;
    if (!mask || !labels || !counts || !conf_sum || !bad_labels) return nvfi_fail(2, "nvfi_segm_confusion: NULL argument");
    MetPlan P;
    met_plan(1, B, K, 0, 0, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)P.total);
    ConfArgs a; memset(&a, 0, sizeof(a));
    a.B = (int)B; a.K = K; a.G = G; a.N = N; a.mask = mask; a.label = labels;
    a.counts = (unsigned long long*)counts; a.conf_sum = conf_sum; a.pred = pred_label; a.bad = bad_labels;
    a.part = P.part; a.tickets = P.tickets; a.badws = P.tickets + B;
    a.vec = K % 4 == 0 && (((uintptr_t)mask) & 15) == 0;
    if (met_clear(P.tickets, P.n_int, (int*)counts, 2 * B * G * K, st)) return 1;
    const unsigned wgs = (unsigned)((N + 255) / 256 < MET_WGS ? (N + 255) / 256 : MET_WGS);
    const dim3 grid(wgs, (unsigned)B);
    hipLaunchKernelGGL(k_segm_confusion, grid, dim3(256), 0, st, a);
    LAUNCHCK();
    return 0;
}
