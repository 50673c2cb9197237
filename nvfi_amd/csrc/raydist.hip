// raydist.hip - distortion loss on the ray weights of a render (Mip-NeRF 360, eq. 15, for the piecewise-constant weights of a ray whose samples
// are equally spaced: every built sampling path, k_sample non-NDC).  The reference has no such term; the render backward has its input (g_weights).
//   D_r  = delta [ sum_i sum_j w_i w_j |i - j| + (1/3) sum_i w_i^2 ] = delta [ 2 sum_i w_i A_i + (1/3) sum_i w_i^2 ]
//   loss = (1/R) sum_r D_r,     d loss / d w_i = (delta / R) [ 2 (A_i + B_i) + (2/3) w_i ]
//   A_i  = sum_{j<i} (i - j) w_j = exclusive prefix sum of the inclusive prefix sum of w;  B_i the same from the right.  Sums of non-negative terms:
//          nothing of the size of i * W is subtracted.
// k_ray_dist   one wave per ray, four rays per 256-thread workgroup, lanes stride the ray in chunks of 64 with carries between the chunks
//              (k_weights_fwd's layout and its shuffle scan).  The forward sweep forms A, sums w A and w^2 in fp64 and writes the left half
//              of the gradient, (delta / R) [2 A_i + (2/3) w_i]; the reverse sweep RE-READS the weights (L2), forms B with the mirrored scan and
//              adds 2 (delta / R) B_i - element j by the lane that wrote it.  Nothing is held per chunk, so any S >= 1 runs on one code path (held in
//              registers, a ray of 1024 samples is 16 chunks of w and A per lane and S gets a cap).  g_weights must not overlap weights.
// k_ray_mean   second launch of ONE workgroup over the R fp64 per-ray values in the workspace, summed in a fixed order: two calls give the same bits.
// No LDS in the scans, no atomics, no memset, no host synchronisation: the call can be captured in a hipGraph.
#include "reduce.h"

#define RD_MEAN_THREADS 1024

__global__ __launch_bounds__(256) void k_ray_dist(int64_t R, int S, const float* __restrict__ weights, float delta, float grad_scale,
                                                  const float* __restrict__ grad_scale_dev, double inv_R, double* __restrict__ dr,
                                                  float* __restrict__ per_ray, float* __restrict__ g_weights) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                // (whole waves leave: the shuffles below see full waves)
    const float* w = weights + r * (int64_t)S;
    float* g = g_weights ? g_weights + r * (int64_t)S : nullptr;
    const double gs = (double)grad_scale * (grad_scale_dev ? (double)grad_scale_dev[0] : 1.0) * (double)delta * inv_R;
    const float k2 = (float)(2.0 * gs), k23 = (float)(gs * 2.0 / 3.0);
    float cW = 0.f, cA = 0.f;                          // carries: sum of w, sum of the inclusive sums, over the chunks in front
    double s1 = 0.0, s2 = 0.0;
    for (int j0 = 0; j0 < S; j0 += 64) {               // wave-uniform trip count
        const int j = j0 + lane;
        const float x = j < S ? w[j] : 0.f;
        float p = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(p, o); if (lane >= o) p += t; }
        const float winc = cW + p;                     // inclusive prefix sum of w at j
        float q = winc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(q, o); if (lane >= o) q += t; }
        float e = __shfl_up(q, 1);
        if (lane == 0) e = 0.f;
        const float A = cA + e;
        cW = __shfl(winc, 63);
        cA += __shfl(q, 63);                           // (lanes past S add to it in the last chunk only: nobody reads it afterwards)
        s1 += (double)x * (double)A;
        s2 += (double)x * (double)x;
        if (g && j < S) g[j] = k2 * A + k23 * x;       // the left half of the gradient; the reverse sweep's SAME lane adds the right half
    }
    if (dr || per_ray) {
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) {
            const double D = (double)delta * (2.0 * s1 + s2 / 3.0);
            if (dr) dr[r] = D;
            if (per_ray) per_ray[r] = (float)D;
        }
    }
    if (!g) return;
    cW = 0.f;
    float cB = 0.f;
    for (int j0 = (S - 1) / 64 * 64; j0 >= 0; j0 -= 64) {
        const int j = j0 + lane;
        const float x = j < S ? w[j] : 0.f;            // re-read (L2); 0 past S: the suffix sums there are 0
        float p = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_down(p, o); if (lane + o < 64) p += t; }
        const float wsuf = cW + p;                     // inclusive suffix sum of w at j
        float q = wsuf;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_down(q, o); if (lane + o < 64) q += t; }
        float e = __shfl_down(q, 1);
        if (lane == 63) e = 0.f;
        const float B = cB + e;
        cW = __shfl(wsuf, 0);
        cB += __shfl(q, 0);
        if (j < S) g[j] += k2 * B;                     // (this thread's own store of the forward sweep: program order, no fence)
    }
}

// loss[0] = inv_R * sum of dr[0..R): every thread sums its stride, then the workgroup's ordered sum (reduce.h)
__global__ __launch_bounds__(RD_MEAN_THREADS) void k_ray_mean(int64_t R, const double* __restrict__ dr, double inv_R, float* __restrict__ loss) {
    __shared__ double part[RD_MEAN_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < R; i += RD_MEAN_THREADS) s += dr[i];
    block_sum_ordered<RD_MEAN_THREADS / 64, 1>(&s, part, tid & 63, tid >> 6);
    if (tid == 0) loss[0] = (float)(s * inv_R);
}

static int64_t rd_workspace_bytes(int64_t R) { return align_up((R > 0 ? R : 1) * (int64_t)sizeof(double), 256); }

extern "C" int nvfi_ray_distortion_workspace_bytes(int64_t R, int64_t* bytes) {
    if (R < 0 || !bytes) return nvfi_fail(2, "nvfi_ray_distortion_workspace_bytes: R must not be negative, bytes must not be NULL");
    *bytes = rd_workspace_bytes(R);
    return 0;
}

extern "C" int nvfi_ray_distortion(int64_t R, int S, const float* weights, float delta, float grad_scale, const float* grad_scale_dev,
                                   float* loss, float* per_ray, float* g_weights, void* workspace, int64_t workspace_bytes, void* stream) {
    if (R < 0) return nvfi_fail(2, "nvfi_ray_distortion: R must not be negative");
    if (S < 1) return nvfi_fail(2, "nvfi_ray_distortion: S = %d, a ray has at least one sample", S);
    if (R > 0 && !weights) return nvfi_fail(2, "nvfi_ray_distortion: weights must not be NULL");
    if ((R + 3) / 4 > 0x7fffffffLL) return nvfi_fail(2, "nvfi_ray_distortion: R = %lld is more than one grid holds", (long long)R);
    const bool need_ws = loss && R > 0;                // only the mean reads the workspace: the fp64 per-ray values of this call
    if (need_ws && (!workspace || workspace_bytes < rd_workspace_bytes(R)))
        return nvfi_fail(4, "nvfi_ray_distortion: workspace of %lld bytes, %lld needed", (long long)(workspace ? workspace_bytes : 0), (long long)rd_workspace_bytes(R));
    if (need_ws && ((uintptr_t)workspace & 7))
        return nvfi_fail(4, "nvfi_ray_distortion: the workspace holds doubles and must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* dr = need_ws ? reinterpret_cast<double*>(workspace) : nullptr;
    const double inv_R = R > 0 ? 1.0 / (double)R : 0.0;
    if (R > 0 && (loss || per_ray || g_weights)) {
        const dim3 grid((unsigned)((R + 3) / 4)), block(256);
        hipLaunchKernelGGL(k_ray_dist, grid, block, 0, st, R, S, weights, delta, grad_scale, grad_scale_dev, inv_R, dr, per_ray, g_weights);
        LAUNCHCK();
    }
    if (loss) {                                        // R == 0: an empty sum, loss = 0
        hipLaunchKernelGGL(k_ray_mean, dim3(1), dim3(RD_MEAN_THREADS), 0, st, R, dr, inv_R, loss);
        LAUNCHCK();
    }
    return 0;
}
