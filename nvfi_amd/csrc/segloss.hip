// segloss.hip - the objective of the MaskField training step (train_segm.py:182-202; utils/seg_loss.py: dynamic_loss with fit_motion_svd_batch,
// smooth_loss, entropy_loss) on the GPU: nvfi_knn_self and nvfi_segloss of include/nvfi_hip.h.
//
//   nvfi_knn_self   k_seg_bounds      min / max of the cloud in two stages; the last workgroup lays out the cell grid (cell side >= sqrt(radius))
//                   k_seg_cell_count  cell of every point + histogram          \
//                   k_seg_scan        cell starts (one workgroup)               > counting sort of the points by cell
//                   k_seg_cell_fill   points in cell order (x, y, z, index)    /
//                   k_seg_knn         one thread per point: 27 cells = 9 contiguous runs, k-entry insertion list in registers, ordered by
//                                     (squared distance, index) - a total order, so the list does not depend on the order within a cell
//                   k_seg_scan / k_seg_rev_fill / k_seg_rev_sort   reverse adjacency lists: counting sort of the live edges by target, every
//                                     list then sorted by edge number (the fill's cursor is an atomic: its order is not repeatable, the sort's is)
//   nvfi_segloss    k_seg_moments1    per object: sum m, sum m pc, sum m pc2 -> weighted means (two stages, last workgroup)
//                   k_seg_moments2    per object: S = sum m (pc - mu1)(pc2 - mu2)^T, centred; the last workgroup sums the partials in workgroup
//                                     order in fp64 and runs the K 3x3 SVDs (one-sided Jacobi, fp64, one lane each) -> R, t
//                   k_seg_points      one thread per point: q = sum_k m_k (R_k pc + t_k), the three loss terms and the whole row of d/d mask
//                                     (both ends of every kNN edge through the reverse lists: a gather, no float atomics); losses in two stages
// House rules and the in-launch hand-off (publish, last_arrival, read_published): reduce.h.  Every ticket here counts the launch's gridDim.x workgroups.
#include <limits.h>
#include <string.h>
#include "reduce.h"

#define SEG_MAX_CELLS 65536      // cap of the cell grid: beyond it the cell side grows (the search stays exact, it only visits more points)
#define SEG_MAX_AXIS 256         // cells per axis: cell coordinates stay far below the 2^-24 relative rounding of their computation
#define SEG_WGS 128              // workgroups (= partial sums per value) of the grid-stride reductions
#define SEG_MAX_OBJ 16
#define SEG_MAX_NN 16
#define SEG_CELL_MARGIN 1.002f   // cell side over sqrt(radius): two points within the radius never sit more than one cell apart after rounding

struct SegGrid { float lo[3]; float inv; int n[3]; int ncell; };

__device__ __forceinline__ int seg_axis_cell(float x, float lo, float inv, int n) {
    const float c = floorf((x - lo) * inv);
    return (int)fminf(fmaxf(c, 0.f), (float)(n - 1));      // (fmaxf drops a NaN: such a point sorts into cell 0 and has no neighbours)
}
__device__ __forceinline__ int seg_cell(const SegGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = seg_axis_cell(x, g.lo[0], g.inv, g.n[0]); cy = seg_axis_cell(y, g.lo[1], g.inv, g.n[1]); cz = seg_axis_cell(z, g.lo[2], g.inv, g.n[2]);
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}

// ---------------------------------------------------------------- kNN: bounds and cell grid
__global__ __launch_bounds__(256) void k_seg_bounds(int N, const float* __restrict__ pc, float radius, float* partial, int* ticket, SegGrid* grid) {
    __shared__ float red[4][6];
    __shared__ float fin[6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = pc[3 * (int64_t)i + c]; b[c] = fminf(b[c], v); b[3 + c] = fmaxf(b[3 + c], v); }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const float u = __shfl_xor(b[c], o); b[c] = c < 3 ? fminf(b[c], u) : fmaxf(b[c], u); }
        if (lane == 0) red[wv][c] = b[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = red[0][c];
        for (int w = 1; w < 4; ++w) v = c < 3 ? fminf(v, red[w][c]) : fmaxf(v, red[w][c]);
        publish(partial + blockIdx.x * 6 + c, v);
    }
    if (!last_arrival(ticket, (int)gridDim.x)) return;
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = read_published(partial + c);
        for (int w = 1; w < (int)gridDim.x; ++w) { const float u = read_published(partial + w * 6 + c); v = c < 3 ? fminf(v, u) : fmaxf(v, u); }
        fin[c] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ext[3], emax = 0.f;
        for (int c = 0; c < 3; ++c) { ext[c] = fin[3 + c] - fin[c]; if (!(ext[c] >= 0.f)) ext[c] = 0.f; if (!(ext[c] < 1e30f)) ext[c] = 1e30f; emax = fmaxf(emax, ext[c]); }
        float h = fmaxf(sqrtf(fmaxf(radius, 0.f)) * SEG_CELL_MARGIN, fmaxf(emax * (1.f / 4096.f), 1e-30f));
        int n[3];
        for (int it = 0; it < 64; ++it) {       // the cap: grow the cell side until the grid fits
            for (int c = 0; c < 3; ++c) { float nf = fminf(floorf(ext[c] / h) + 1.f, (float)SEG_MAX_AXIS); if (!(nf >= 1.f)) nf = 1.f; n[c] = (int)nf; }
            if ((int64_t)n[0] * n[1] * n[2] <= SEG_MAX_CELLS) break;
            h *= 1.25f;
        }
        while ((int64_t)n[0] * n[1] * n[2] > SEG_MAX_CELLS) { int c = n[0] >= n[1] && n[0] >= n[2] ? 0 : (n[1] >= n[2] ? 1 : 2); n[c] = (n[c] + 1) / 2; }   // (never after 64 x 1.25)
        SegGrid g;
        for (int c = 0; c < 3; ++c) { g.lo[c] = fin[c]; g.n[c] = n[c]; }
        g.inv = 1.f / h; g.ncell = n[0] * n[1] * n[2];
        *grid = g;
    }
}

__global__ __launch_bounds__(256) void k_seg_cell_count(int N, const float* __restrict__ pc, const SegGrid* grid, int* cellid, int* count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const SegGrid g = *grid;
    int cx, cy, cz;
    const int c = seg_cell(g, pc[3 * (int64_t)i], pc[3 * (int64_t)i + 1], pc[3 * (int64_t)i + 2], cx, cy, cz);
    cellid[i] = c;
    atomicAdd(count + c, 1);
}

// exclusive scan of n ints by ONE workgroup of 1024 threads; out[n] = total
__global__ __launch_bounds__(1024) void k_seg_scan(const int* __restrict__ in, int* __restrict__ out, int n) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? in[i] : 0;
        int s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(s, o); if (lane >= o) s += u; }
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int x = wsum[w]; if (w < wv) pre += x; tot += x; }
        if (i < n) out[i] = carry + pre + s - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// count[c] counts down: the slots of a cell are handed out from its end (the order within a cell is not repeatable, and nothing depends on it)
__global__ __launch_bounds__(256) void k_seg_cell_fill(int N, const float* __restrict__ pc, const int* __restrict__ cellid, const int* __restrict__ start,
                                                       int* count, float4* sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int c = cellid[i];
    const int pos = start[c] + atomicSub(count + c, 1) - 1;
    if (pos >= 0 && pos < N) sorted[pos] = make_float4(pc[3 * (int64_t)i], pc[3 * (int64_t)i + 1], pc[3 * (int64_t)i + 2], __int_as_float(i));
}

template <int KT>
__global__ __launch_bounds__(256) void k_seg_knn(int N, const float4* __restrict__ sorted, const int* __restrict__ start, const SegGrid* grid,
                                                 int k, float radius, int* __restrict__ idx, float* __restrict__ d2out, int* indeg) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const SegGrid g = *grid;
    const float4 q = sorted[s];
    const int qi = __float_as_int(q.w);
    if (qi < 0 || qi >= N) return;
    int cx, cy, cz;
    seg_cell(g, q.x, q.y, q.z, cx, cy, cz);
    float bd[KT]; int bi[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { bd[j] = INFINITY; bi[j] = INT_MAX; }
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.n[0] - 1);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.n[2] - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.n[1] - 1); ++y) {
            const int row = (z * g.n[1] + y) * g.n[0];
            const int b = max(start[row + x0], 0), e = min(start[row + x1 + 1], N);
            for (int c = b; c < e; ++c) {
                const float4 p = sorted[c];
                const float ex = q.x - p.x, ey = q.y - p.y, ez = q.z - p.z;
                float td = (ex * ex + ey * ey) + ez * ez;
                int ti = __float_as_int(p.w);
                if (!(td <= radius)) continue;      // beyond the radius (or NaN): such a slot is replaced by slot 0 anyway
                if (!(td < bd[KT - 1] || (td == bd[KT - 1] && ti < bi[KT - 1]))) continue;
#pragma unroll
                for (int j = 0; j < KT; ++j) {      // insertion: the entry sinks to its place, everything behind it moves one slot down
                    const bool lt = td < bd[j] || (td == bd[j] && ti < bi[j]);
                    const float od = bd[j]; const int oi = bi[j];
                    bd[j] = lt ? td : od; bi[j] = lt ? ti : oi;
                    td = lt ? od : td; ti = lt ? oi : ti;
                }
            }
        }
    const int i0 = (bi[0] < 0 || bi[0] >= N) ? qi : bi[0];
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        if (j >= k) continue;
        const bool have = bi[j] >= 0 && bi[j] < N;
        const int t = have ? bi[j] : i0;
        idx[(int64_t)qi * k + j] = t;
        if (d2out) d2out[(int64_t)qi * k + j] = have ? bd[j] : INFINITY;
        if (indeg && t != qi) atomicAdd(indeg + t, 1);
    }
}

__global__ __launch_bounds__(256) void k_seg_rev_fill(int N, int k, const int* __restrict__ idx, const int* __restrict__ rev_start, int* indeg, int* rev_edge) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * k) return;
    const int n = e / k, t = idx[e];
    if (t == n || t < 0 || t >= N) return;
    const int pos = rev_start[t] + atomicSub(indeg + t, 1) - 1;
    if (pos >= 0 && pos < N * k) rev_edge[pos] = e;
}
// every list ascending by edge number (Shell sort, gaps 2^j - 1: a plain insertion sort for the usual handful of entries, O(d^1.5) for the
// long list of a point that a whole cluster of duplicates has chosen)
__global__ __launch_bounds__(256) void k_seg_rev_sort(int N, const int* __restrict__ rev_start, int* rev_edge) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const int b = rev_start[t], d = rev_start[t + 1] - b;
    int* L = rev_edge + b;
    int gap = 1;
    while (gap * 2 + 1 < d) gap = gap * 2 + 1;
    for (; gap > 0; gap >>= 1)
        for (int i = gap; i < d; ++i) {
            const int v = L[i];
            int j = i;
            while (j >= gap && L[j - gap] > v) { L[j] = L[j - gap]; j -= gap; }
            L[j] = v;
        }
}

// ---------------------------------------------------------------- rigid fit
template <int KP> __device__ __forceinline__ void seg_load_row(const float* __restrict__ mask, int64_t n, int K, bool vec, float* m) {
    if (vec) {          // K == KP, rows 16-byte aligned: K = 8 is two 16-byte loads
#pragma unroll
        for (int q4 = 0; q4 < KP / 4; ++q4) { const float4 v = ld4(mask + n * KP + 4 * q4); m[4 * q4] = v.x; m[4 * q4 + 1] = v.y; m[4 * q4 + 2] = v.z; m[4 * q4 + 3] = v.w; }
    } else {
#pragma unroll
        for (int c = 0; c < KP; ++c) m[c] = c < K ? mask[n * K + c] : 0.f;
    }
}
struct SegArgs {
    int N, K, k; bool vec;
    const float* pc; const float* flow; const float* mask;
    const int* idx; const int* rev_start; const int* rev_edge;
    int loss_norm; float eps, wd, ws, we, gscale; int accumulate;
    float* gmask; float* losses; float* R; float* t; float* pct;
    float* part1; float* part2; float* part3; float* mu; int* tickets;
};

// NV values per thread summed over the workgroup and published as this workgroup's partials.  Not reduce.h's block_sum_ordered: the four wave
// sums are added PAIRWISE in fp32 (k_seg_points' line below does the same) - the sequential order gives other bits
template <int NV> __device__ __forceinline__ void seg_block_publish(float* acc, float* red /* [4][NV] */, float* partial) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) { const float s = wave_sum(acc[v]); if (lane == 0) red[wv * NV + v] = s; }
    __syncthreads();
    for (int v = threadIdx.x; v < NV; v += 256) publish(partial + (int64_t)blockIdx.x * NV + v, (red[v] + red[NV + v]) + (red[2 * NV + v] + red[3 * NV + v]));
}

template <int KP>
__global__ __launch_bounds__(256) void k_seg_moments1(SegArgs a) {
    __shared__ float red[4 * 7 * KP];
    __shared__ double fin[7 * KP];
    float acc[7 * KP];
#pragma unroll
    for (int v = 0; v < 7 * KP; ++v) acc[v] = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.N; i += gridDim.x * 256) {
        float m[KP];
        seg_load_row<KP>(a.mask, i, a.K, a.vec, m);
        float p[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = a.pc[3 * (int64_t)i + c]; p[3 + c] = p[c] + a.flow[3 * (int64_t)i + c]; }
#pragma unroll
        for (int o = 0; o < KP; ++o) {
            acc[7 * o] += m[o];
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[7 * o + 1 + c] += m[o] * p[c];
        }
    }
    seg_block_publish<7 * KP>(acc, red, a.part1);
    if (!last_arrival(a.tickets, (int)gridDim.x)) return;
    for (int v = threadIdx.x; v < 7 * KP; v += 256) {
        double s = 0.0;
        for (int w = 0; w < (int)gridDim.x; ++w) s += (double)read_published(a.part1 + (int64_t)w * 7 * KP + v);
        fin[v] = s;
    }
    __syncthreads();
    if (threadIdx.x < KP) {      // mean = weighted sum / weight: 0 / 0 = NaN for an empty object, which the fit turns into the identity
        const int o = threadIdx.x;
        const float sm = (float)fin[7 * o];
        for (int c = 0; c < 6; ++c) a.mu[8 * o + c] = (float)fin[7 * o + 1 + c] / sm;
        a.mu[8 * o + 6] = sm; a.mu[8 * o + 7] = 0.f;
    }
}

// R = V diag(1, 1, det(V U^T)) U^T of S = U diag(s) V^T, written as v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T: the third pair enters only through
// the two leading ones, whatever sign an SVD gives it.  One-sided Jacobi on the columns of G = S V.
__device__ void seg_rotation_from_S(const double* S, double* R) {
    double G[3][3], V[3][3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { G[r][c] = S[3 * r + c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double al = 0.0, be = 0.0, ga = 0.0;
            for (int r = 0; r < 3; ++r) { al += G[r][p] * G[r][p]; be += G[r][q] * G[r][q]; ga += G[r][p] * G[r][q]; }
            if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
            rotated = true;
            const double ze = (be - al) / (2.0 * ga);
            const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
            const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
            for (int r = 0; r < 3; ++r) {
                const double gp = G[r][p], gq = G[r][q], vp = V[r][p], vq = V[r][q];
                G[r][p] = cs * gp - sn * gq; G[r][q] = sn * gp + cs * gq;
                V[r][p] = cs * vp - sn * vq; V[r][q] = sn * vp + cs * vq;
            }
        }
        if (!rotated) break;
    }
    double sg[3];
    for (int c = 0; c < 3; ++c) sg[c] = sqrt(G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c]);
    int i1 = sg[0] >= sg[1] && sg[0] >= sg[2] ? 0 : (sg[1] >= sg[2] ? 1 : 2);
    int ia = (i1 + 1) % 3, ib = (i1 + 2) % 3;
    int i2 = sg[ia] >= sg[ib] ? ia : ib;
    for (int r = 0; r < 9; ++r) R[r] = (r % 4 == 0) ? 1.0 : 0.0;
    if (!(sg[i1] > 0.0)) return;                                    // S = 0: nothing to fit
    double u1[3], u2[3], v1[3], v2[3];
    for (int r = 0; r < 3; ++r) { u1[r] = G[r][i1] / sg[i1]; v1[r] = V[r][i1]; v2[r] = V[r][i2]; }
    if (sg[i2] > 1e-150 * sg[i1]) { for (int r = 0; r < 3; ++r) u2[r] = G[r][i2] / sg[i2]; }
    else {                                                           // rank one: any unit vector across u1 (the fit is not unique there)
        const int sm = fabs(u1[0]) <= fabs(u1[1]) && fabs(u1[0]) <= fabs(u1[2]) ? 0 : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
        double e[3] = {0.0, 0.0, 0.0}; e[sm] = 1.0;
        u2[0] = u1[1] * e[2] - u1[2] * e[1]; u2[1] = u1[2] * e[0] - u1[0] * e[2]; u2[2] = u1[0] * e[1] - u1[1] * e[0];
        const double nn = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        for (int r = 0; r < 3; ++r) u2[r] /= nn;
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = v1[r] * u1[c] + v2[r] * u2[c] + v3[r] * u3[c];
}

template <int KP>
__global__ __launch_bounds__(256) void k_seg_moments2(SegArgs a) {
    __shared__ float red[4 * 9 * KP];
    __shared__ double fin[9 * KP];
    __shared__ float smu[8 * KP];
    for (int v = threadIdx.x; v < 8 * KP; v += 256) smu[v] = a.mu[v];
    __syncthreads();
    float acc[9 * KP];
#pragma unroll
    for (int v = 0; v < 9 * KP; ++v) acc[v] = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.N; i += gridDim.x * 256) {
        float m[KP];
        seg_load_row<KP>(a.mask, i, a.K, a.vec, m);
        float p[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = a.pc[3 * (int64_t)i + c]; p[3 + c] = p[c] + a.flow[3 * (int64_t)i + c]; }
#pragma unroll
        for (int o = 0; o < KP; ++o) {
            if (o >= a.K) continue;
            float d1[3], d2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { d1[c] = p[c] - smu[8 * o + c]; d2[c] = m[o] * (p[3 + c] - smu[8 * o + 3 + c]); }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[9 * o + 3 * r + c] += d1[r] * d2[c];
        }
    }
    seg_block_publish<9 * KP>(acc, red, a.part2);
    if (!last_arrival(a.tickets + 1, (int)gridDim.x)) return;
    for (int v = threadIdx.x; v < 9 * KP; v += 256) {
        double s = 0.0;
        for (int w = 0; w < (int)gridDim.x; ++w) s += (double)read_published(a.part2 + (int64_t)w * 9 * KP + v);
        fin[v] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.K) {
        const int o = threadIdx.x;
        double R[9], t[3] = {0.0, 0.0, 0.0};
        bool nan = false;
        for (int r = 0; r < 9; ++r) nan |= !(fin[9 * o + r] == fin[9 * o + r]);
        if (nan) { for (int r = 0; r < 9; ++r) R[r] = (r % 4 == 0) ? 1.0 : 0.0; }      // seg_loss.py:34-38: an ill-posed object keeps the identity
        else {
            seg_rotation_from_S(fin + 9 * o, R);
            for (int r = 0; r < 3; ++r)
                t[r] = (double)smu[8 * o + 3 + r] - (R[3 * r] * (double)smu[8 * o] + R[3 * r + 1] * (double)smu[8 * o + 1] + R[3 * r + 2] * (double)smu[8 * o + 2]);
        }
        for (int r = 0; r < 9; ++r) a.R[9 * o + r] = (float)R[r];
        for (int r = 0; r < 3; ++r) a.t[3 * o + r] = (float)t[r];
    }
}

// ---------------------------------------------------------------- per-point pass: the three losses and d / d mask
template <int KP>
__global__ __launch_bounds__(256) void k_seg_points(SegArgs a) {
    __shared__ float sR[12 * KP];
    __shared__ float red[4 * 3];
    const bool rigid = a.flow != nullptr, smooth = a.idx != nullptr;
    if (rigid) {
        for (int v = threadIdx.x; v < 12 * a.K; v += 256) { const int o = v / 12, r = v % 12; sR[v] = r < 9 ? a.R[9 * o + r] : a.t[3 * o + r - 9]; }
    }
    __syncthreads();
    const int n = blockIdx.x * 256 + threadIdx.x;
    float acc[3] = {0.f, 0.f, 0.f};
    if (n < a.N) {
        float m[KP], g[KP];
        seg_load_row<KP>(a.mask, n, a.K, a.vec, m);
        const float invN = 1.f / (float)a.N;
#pragma unroll
        for (int o = 0; o < KP; ++o) g[o] = 0.f;
        if (rigid) {
            float p[3], p2[3], T[KP][3], q[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) { p[c] = a.pc[3 * (int64_t)n + c]; p2[c] = p[c] + a.flow[3 * (int64_t)n + c]; }
#pragma unroll
            for (int o = 0; o < KP; ++o) {
                if (o >= a.K) continue;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    T[o][r] = ((sR[12 * o + 3 * r] * p[0] + sR[12 * o + 3 * r + 1] * p[1]) + sR[12 * o + 3 * r + 2] * p[2]) + sR[12 * o + 9 + r];
                    q[r] += m[o] * T[o][r];
                }
            }
            const float r0 = q[0] - p2[0], r1 = q[1] - p2[1], r2 = q[2] - p2[2];
            const float nr = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
            acc[0] = nr;
            const float s = nr > 0.f ? a.wd * invN / nr : 0.f;       // the norm's gradient at 0 is 0, as in torch
#pragma unroll
            for (int o = 0; o < KP; ++o) {
                if (o >= a.K) continue;
                g[o] += s * ((r0 * T[o][0] + r1 * T[o][1]) + r2 * T[o][2]);
            }
            if (a.pct) { a.pct[3 * (int64_t)n] = q[0]; a.pct[3 * (int64_t)n + 1] = q[1]; a.pct[3 * (int64_t)n + 2] = q[2]; }
        }
        {   // entropy: -sum m log(max(m, eps))
            float e = 0.f;
#pragma unroll
            for (int o = 0; o < KP; ++o) {
                if (o >= a.K) continue;
                const float lm = logf(fmaxf(m[o], a.eps));
                e -= m[o] * lm;
                g[o] -= a.we * invN * (lm + (m[o] > a.eps ? 1.f : 0.f));
            }
            acc[2] = e;
        }
        if (smooth) {
            const float ws = a.ws / ((float)a.N * (float)a.k);
            float sl = 0.f;
            // both ends of every edge: the point's own k edges (they count in the loss), then the edges that point AT it (gradient only)
            const int nin = a.rev_start ? a.rev_start[n + 1] - a.rev_start[n] : 0;
            const int rb = a.rev_start ? a.rev_start[n] : 0;
            for (int j = 0; j < a.k + nin; ++j) {
                const bool own = j < a.k;
                int o_ = own ? a.idx[(int64_t)n * a.k + j] : a.rev_edge[rb + j - a.k] / a.k;
                if (o_ == n || o_ < 0 || o_ >= a.N) continue;        // a replaced slot (the point itself): |0| = 0, gradient 0
                float mo[KP], d[KP];
                seg_load_row<KP>(a.mask, o_, a.K, a.vec, mo);
                float nrm = 0.f;
                if (a.loss_norm == 1) {
#pragma unroll
                    for (int o = 0; o < KP; ++o) { d[o] = m[o] - mo[o]; nrm += fabsf(d[o]); d[o] = d[o] > 0.f ? 1.f : (d[o] < 0.f ? -1.f : 0.f); }
                } else {
#pragma unroll
                    for (int o = 0; o < KP; ++o) { d[o] = m[o] - mo[o]; nrm += d[o] * d[o]; }
                    nrm = sqrtf(nrm);
                    const float inv = nrm > 0.f ? 1.f / nrm : 0.f;
#pragma unroll
                    for (int o = 0; o < KP; ++o) d[o] *= inv;
                }
                if (own) sl += nrm;
                // one formula for both ends: d |m_n - m_o| / d m_n = d |m_o - m_n| / d m_n = d (the norm is even in its argument)
#pragma unroll
                for (int o = 0; o < KP; ++o) g[o] += ws * d[o];
            }
            acc[1] = sl;
        }
        if (a.gmask) {
#pragma unroll
            for (int o = 0; o < KP; ++o) {
                if (o >= a.K) continue;
                float* gp = a.gmask + (int64_t)n * a.K + o;
                const float v = a.gscale * g[o];
                *gp = a.accumulate ? *gp + v : v;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float s = wave_sum(acc[c]); if (lane == 0) red[wv * 3 + c] = s; }
    __syncthreads();
    if (threadIdx.x < 3) publish(a.part3 + (int64_t)blockIdx.x * 3 + threadIdx.x, (red[threadIdx.x] + red[3 + threadIdx.x]) + (red[6 + threadIdx.x] + red[9 + threadIdx.x]));
    if (!last_arrival(a.tickets + 2, (int)gridDim.x)) return;
    if (wv == 0) {
        float total = 0.f;
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int w = lane; w < (int)gridDim.x; w += 64) s += (double)read_published(a.part3 + (int64_t)w * 3 + c);
            s = wave_sum(s);
            const double den = c == 1 ? (double)a.N * (double)a.k : (double)a.N;
            const float v = (c == 0 && !rigid) || (c == 1 && !smooth) ? 0.f : (float)(s / den);
            if (lane == 0) a.losses[c] = v;
            total += (c == 0 ? a.wd : (c == 1 ? a.ws : a.we)) * v;
        }
        if (lane == 0) a.losses[3] = total;
    }
}

// ---------------------------------------------------------------- host
static int seg_wgs(int64_t N) { return (int)((N + 255) / 256 < SEG_WGS ? (N + 255) / 256 : SEG_WGS); }
struct KnnPlan { SegGrid* grid; float* bpart; int* zero0; int* ticket; int* count; int* indeg; int64_t zero_bytes; int* start; int* cellid; float4* sorted; int64_t total; };
static void plan_knn(int64_t N, void* ws, KnnPlan* P) {
    Bump B{(char*)ws, 0, 0};
    P->grid = B.take<SegGrid>(1);
    P->bpart = B.take<float>(6 * SEG_WGS);
    P->zero0 = B.take<int>(0);
    P->ticket = B.take<int>(64);
    P->count = B.take<int>(SEG_MAX_CELLS);
    P->indeg = B.take<int>(N);
    P->zero_bytes = B.off - (int64_t)((char*)P->zero0 - (char*)ws);
    P->start = B.take<int>(SEG_MAX_CELLS + 1);
    P->cellid = B.take<int>(N);
    P->sorted = B.take<float4>(N);
    P->total = align_up(B.off, 256);
}
struct LossPlan { int* tickets; float* part1; float* part2; float* part3; float* mu; int64_t total; };
static void plan_loss(int64_t N, void* ws, LossPlan* P) {
    Bump B{(char*)ws, 0, 0};
    P->tickets = B.take<int>(64);
    P->part1 = B.take<float>(SEG_WGS * 7 * SEG_MAX_OBJ);
    P->part2 = B.take<float>(SEG_WGS * 9 * SEG_MAX_OBJ);
    P->part3 = B.take<float>(3 * ((N + 255) / 256));
    P->mu = B.take<float>(8 * SEG_MAX_OBJ);
    P->total = align_up(B.off, 256);
}
static int seg_sizes_ok(int64_t N, int K, int k) {
    if (N < 0 || N > (1 << 26)) return nvfi_fail(2, "segloss: N = %lld is outside 0..2^26", (long long)N);
    if (K && (K < 2 || K > SEG_MAX_OBJ)) return nvfi_fail(2, "segloss: %d objects (2..%d are supported)", K, SEG_MAX_OBJ);
    if (k && (k < 1 || k > SEG_MAX_NN)) return nvfi_fail(2, "segloss: k = %d neighbours (1..%d are supported)", k, SEG_MAX_NN);
    if (N * (int64_t)(k ? k : 1) > INT_MAX) return nvfi_fail(2, "segloss: N x k = %lld edges do not fit 31 bits", (long long)(N * k));
    return 0;
}
extern "C" int nvfi_segloss_workspace_bytes(int64_t N, int K, int k, int64_t* bytes) {
    if (seg_sizes_ok(N, K, k)) return 2;
    KnnPlan A; LossPlan L;
    plan_knn(N > 0 ? N : 1, nullptr, &A);
    plan_loss(N > 0 ? N : 1, nullptr, &L);
    *bytes = A.total > L.total ? A.total : L.total;
    return 0;
}

extern "C" int nvfi_knn_self(int64_t N, const float* pc, int k, float radius, int32_t* idx, float* d2, int32_t* rev_start, int32_t* rev_edge,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (seg_sizes_ok(N, 0, k) || k < 1) return k < 1 ? nvfi_fail(2, "nvfi_knn_self: k = %d", k) : 2;
    if (!(radius >= 0.f)) return nvfi_fail(2, "nvfi_knn_self: radius %g (it is compared with SQUARED distances and must be >= 0)", (double)radius);
    if ((rev_start == nullptr) != (rev_edge == nullptr)) return nvfi_fail(2, "nvfi_knn_self: rev_start and rev_edge go together");
    if (N == 0) return 0;
    if (!pc || !idx) return nvfi_fail(2, "nvfi_knn_self: NULL points or idx");
    KnnPlan P;
    plan_knn(N, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)P.total);
    const int n = (int)N;
    const unsigned wgN = (unsigned)((N + 255) / 256);
    if (launch_zero(P.zero0, P.zero_bytes, st)) return 1;
    hipLaunchKernelGGL(k_seg_bounds, dim3(seg_wgs(N)), dim3(256), 0, st, n, pc, radius, P.bpart, P.ticket, P.grid);
    hipLaunchKernelGGL(k_seg_cell_count, dim3(wgN), dim3(256), 0, st, n, pc, (const SegGrid*)P.grid, P.cellid, P.count);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(1024), 0, st, (const int*)P.count, P.start, SEG_MAX_CELLS);
    hipLaunchKernelGGL(k_seg_cell_fill, dim3(wgN), dim3(256), 0, st, n, pc, (const int*)P.cellid, (const int*)P.start, P.count, P.sorted);
    int* indeg = rev_start ? P.indeg : nullptr;
    if (k <= 4) hipLaunchKernelGGL(k_seg_knn<4>, dim3(wgN), dim3(256), 0, st, n, (const float4*)P.sorted, (const int*)P.start, (const SegGrid*)P.grid, k, radius, idx, d2, indeg);
    else if (k <= 8) hipLaunchKernelGGL(k_seg_knn<8>, dim3(wgN), dim3(256), 0, st, n, (const float4*)P.sorted, (const int*)P.start, (const SegGrid*)P.grid, k, radius, idx, d2, indeg);
    else hipLaunchKernelGGL(k_seg_knn<16>, dim3(wgN), dim3(256), 0, st, n, (const float4*)P.sorted, (const int*)P.start, (const SegGrid*)P.grid, k, radius, idx, d2, indeg);
    if (rev_start) {
        hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(1024), 0, st, (const int*)P.indeg, rev_start, n);
        hipLaunchKernelGGL(k_seg_rev_fill, dim3((unsigned)((N * k + 255) / 256)), dim3(256), 0, st, n, k, (const int*)idx, (const int*)rev_start, P.indeg, rev_edge);
        hipLaunchKernelGGL(k_seg_rev_sort, dim3(wgN), dim3(256), 0, st, n, (const int*)rev_start, rev_edge);
    }
    LAUNCHCK();
    return 0;
}

template <int KP> static void seg_launch(const SegArgs& a, hipStream_t st) {
    if (a.flow) {
        hipLaunchKernelGGL(k_seg_moments1<KP>, dim3(seg_wgs(a.N)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_seg_moments2<KP>, dim3(seg_wgs(a.N)), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_seg_points<KP>, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, a);
}
extern "C" int nvfi_segloss(int64_t N, int K, const float* pc, const float* flow, const float* mask, int k, const int32_t* idx,
                            const int32_t* rev_start, const int32_t* rev_edge, int loss_norm, float epsilon, float w_dynamic, float w_smooth,
                            float w_entropy, float grad_scale, int accumulate, float* gmask, float* losses4, float* R, float* t,
                            float* pc_transformed, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (seg_sizes_ok(N, K, idx ? k : 0) || K < 2) return K < 2 ? nvfi_fail(2, "nvfi_segloss: %d objects", K) : 2;
    if (idx && loss_norm != 1 && loss_norm != 2) return nvfi_fail(2, "nvfi_segloss: loss_norm %d (1 and 2 are supported)", loss_norm);
    if ((pc == nullptr) != (flow == nullptr)) return nvfi_fail(2, "nvfi_segloss: pc and flow go together (both NULL: no rigid-fit term)");
    if (flow && (!R || !t)) return nvfi_fail(2, "nvfi_segloss: the rigid-fit term needs R and t");
    if (idx && gmask && (!rev_start || !rev_edge)) return nvfi_fail(2, "nvfi_segloss: the smoothness gradient needs the reverse lists of nvfi_knn_self");
    if (!mask || !losses4) return nvfi_fail(2, "nvfi_segloss: NULL mask or losses");
    if (N == 0) return nvfi_fail(2, "nvfi_segloss: no points (the mean of nothing)");
    LossPlan P;
    plan_loss(N, workspace, &P);
    if (!workspace || P.total > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)P.total);
    SegArgs a; memset(&a, 0, sizeof(a));
    a.N = (int)N; a.K = K; a.k = idx ? k : 0;
    a.pc = pc; a.flow = flow; a.mask = mask; a.idx = idx; a.rev_start = rev_start; a.rev_edge = rev_edge;
    a.loss_norm = loss_norm; a.eps = epsilon; a.wd = w_dynamic; a.ws = w_smooth; a.we = w_entropy; a.gscale = grad_scale; a.accumulate = accumulate;
    a.gmask = gmask; a.losses = losses4; a.R = R; a.t = t; a.pct = pc_transformed;
    a.part1 = P.part1; a.part2 = P.part2; a.part3 = P.part3; a.mu = P.mu; a.tickets = P.tickets;
    const int KP = K <= 4 ? 4 : (K <= 8 ? 8 : 16);
    a.vec = K == KP && (((uintptr_t)mask) & 15) == 0;
    if (launch_zero(P.tickets, 64 * sizeof(int), st)) return 1;
    if (KP == 4) seg_launch<4>(a, st); else if (KP == 8) seg_launch<8>(a, st); else seg_launch<16>(a, st);
    LAUNCHCK();
    return 0;
}
