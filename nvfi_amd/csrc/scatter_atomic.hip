// scatter_atomic.hip - plane-gradient scatter with atomics (channel-parallel): what the render backward uses where the sorted-tile scatter
// of scatter.hip does not apply (grid too large for its bins, NVFI_SCATTER_TILES=0) and, in fixed point, under NVFI_DETERMINISTIC.
#include "common.h"
#include "scatter.h"

// One wave walks a few samples; lanes are CHANNELS (x the two x-taps for 24 channels), so every atomic
// instruction adds a contiguous run of one or two texel vectors (96..192 B) instead of 64 scattered words:
// ~14x fewer cache-line atomic operations than one-thread-per-sample scattering.
#define SCATTER_SPW 8
__device__ __forceinline__ float dpp_xor1(float v) { return __shfl_xor(v, 1); }

// DET: the gradient pointers address int64 shadow planes and every contribution is added as a fixed-point integer (2^58 per unit):
// integer addition is associative, so the sums are bit-identical whatever order the atomics arrive in (NVFI_DETERMINISTIC=1).
#define DET_SCALE 288230376151711744.0     /* 2^58: +-32 of range, 3.5e-18 of resolution (2^50 quantised the 1e-10 appearance-plane gradients of an
                                              initial field at 2.5e-3 of their peak: tests/test_gpu_render64.py) */
template <bool DET>
__device__ __forceinline__ void grad_add(float* g, size_t idx, float v) {
    // (a single contribution saturates at the int64 range instead of wrapping; running SUMS beyond +-32 still wrap - test mode)
    if (DET) atomicAdd(reinterpret_cast<unsigned long long*>(g) + idx, (unsigned long long)__double2ll_rn(fmin(fmax((double)v * DET_SCALE, -9.2e18), 9.2e18)));
    else atomicAdd(g + idx, v);
}
__global__ void k_det_finish(const long long* __restrict__ shadow, float* __restrict__ g, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) g[i] += (float)((double)shadow[i] * (1.0 / DET_SCALE));
}
template <int C, bool DET = false>
__global__ __launch_bounds__(256) void k_plane_scatter(ScatterArgs a) {
    const int lane = threadIdx.x & 63;
    const int wg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int count = *a.count;
    const int i0 = wg * SCATTER_SPW;
    if (i0 >= count) return;
    const nvfi_field_desc& f = a.f;
    const float* pl[6]; float* gp[6];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        pl[p] = C == 24 ? f.dps[p] : f.aps[p]; pl[3 + p] = C == 24 ? f.dpt[p] : f.apt[p];
        gp[p] = C == 24 ? a.g.dps[p] : a.g.aps[p]; gp[3 + p] = C == 24 ? a.g.dpt[p] : a.g.apt[p];
    }
    const int ch = C == 24 ? (lane >> 1) : lane;
    const int dx0 = C == 24 ? (lane & 1) : 0;
    const bool lane_on = lane < 48;
#pragma unroll 1
    for (int k = 0; k < SCATTER_SPW; ++k) {
        const int i = i0 + k;
        if (i >= count) break;
        const int n = __builtin_amdgcn_readfirstlane(a.list[i]);
        const float4 q = a.xw[n];
        Bl b[6];
        plane_setups(f, q.x, q.y, q.z, SCHED_TN(a), b);
        float gch;
        if (C == 24) gch = a.gxpre[n];
        else gch = lane_on ? a.gg[(size_t)i * 48 + ch] : 0.f;
        float val[6];
        if (C == 24) {
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const bool my0 = dx0 ? b[p].m1 : b[p].m0, my1 = dx0 ? b[p].m3 : b[p].m2;
                const float wx = dx0 ? b[p].w : b[p].e;
                const size_t o0 = (size_t)(b[p].base + dx0) * C + ch, o1 = o0 + (size_t)b[p].W * C;
                const float v0 = (lane_on && my0) ? pl[p][o0] : 0.f, v1 = (lane_on && my1) ? pl[p][o1] : 0.f;
                const float part = v0 * (wx * b[p].s) + v1 * (wx * b[p].n);
                val[p] = part + dpp_xor1(part);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const size_t o0 = (size_t)b[p].base * C + ch, o1 = o0 + (size_t)b[p].W * C;
                const float v0 = (lane_on && b[p].m0) ? pl[p][o0] : 0.f, v1 = (lane_on && b[p].m1) ? pl[p][o0 + C] : 0.f;
                const float v2 = (lane_on && b[p].m2) ? pl[p][o1] : 0.f, v3 = (lane_on && b[p].m3) ? pl[p][o1 + C] : 0.f;
                val[p] = v0 * (b[p].e * b[p].s) + v1 * (b[p].w * b[p].s) + v2 * (b[p].e * b[p].n) + v3 * (b[p].w * b[p].n);
            }
        }
        // prefix/suffix products: other_p = prod_{k != p} val[k]
        float L[6], Rr[6];
        L[0] = gch; 
#pragma unroll
        for (int p = 1; p < 6; ++p) L[p] = L[p - 1] * val[p - 1];
        Rr[5] = 1.f;
#pragma unroll
        for (int p = 4; p >= 0; --p) Rr[p] = Rr[p + 1] * val[p + 1];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            if (!gp[p] || !lane_on || !((a.plane_mask >> p) & 1)) continue;
            const float o = L[p] * Rr[p];
            if (C == 24) {
                const bool my0 = dx0 ? b[p].m1 : b[p].m0, my1 = dx0 ? b[p].m3 : b[p].m2;
                const float wx = dx0 ? b[p].w : b[p].e;
                const size_t o0 = (size_t)(b[p].base + dx0) * C + ch, o1 = o0 + (size_t)b[p].W * C;
                if (my0) grad_add<DET>(gp[p], o0, (wx * b[p].s) * o);
                if (my1) grad_add<DET>(gp[p], o1, (wx * b[p].n) * o);
            } else {
                const size_t o0 = (size_t)b[p].base * C + ch, o1 = o0 + (size_t)b[p].W * C;
                if (b[p].m0) grad_add<DET>(gp[p], o0, (b[p].e * b[p].s) * o);
                if (b[p].m1) grad_add<DET>(gp[p], o0 + C, (b[p].w * b[p].s) * o);
                if (b[p].m2) grad_add<DET>(gp[p], o1, (b[p].e * b[p].n) * o);
                if (b[p].m3) grad_add<DET>(gp[p], o1 + C, (b[p].w * b[p].n) * o);
            }
        }
    }
}


// Variant with LDS-privatised TIME planes.  The time coordinate is a per-call scalar, so every sample scatters into the
// same two rows of the three time planes (2 x G x C floats each): per-workgroup LDS accumulators absorb that contention
// and are flushed once; space planes keep the coalesced global atomics.  A workgroup handles 24 channels starting at c0
// of planes with CT channels per texel (density: CT=24, one group; appearance: CT=48, two groups on blockIdx.y).
template <int CT>
__global__ __launch_bounds__(1024) void k_plane_scatter_lds(ScatterArgs a) {
    extern __shared__ __attribute__((aligned(16))) float acc_lds[];   // [3 planes][2 rows][gmax][24]
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int c0 = blockIdx.y * 24;
    const int gmax = a.gmax;
    for (int k = threadIdx.x; k < 6 * gmax * 24; k += blockDim.x) acc_lds[k] = 0.f;
    __syncthreads();
    const int count = *a.count;
    const float* pl[6]; float* gp[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        pl[p] = CT == 24 ? f.dps[p] : f.aps[p]; pl[3 + p] = CT == 24 ? f.dpt[p] : f.apt[p];
        gp[p] = CT == 24 ? a.g.dps[p] : a.g.aps[p];
    }
    const int ch = lane >> 1, dx0 = lane & 1;
    const bool lane_on = lane < 48;
    const int wave_global = __builtin_amdgcn_readfirstlane(blockIdx.x * nwv + wv), wave_total = gridDim.x * nwv;
    // two samples per trip: the dependent chain list -> position -> taps is pure latency, so both chains are issued together
    constexpr int U = 2;
    // each wave walks a contiguous run of the (ray-ordered) list: neighbouring samples share texels, so their atomics
    // stay in one wave / one XCD's L2 instead of bouncing the same lines between XCDs
#ifdef NVFI_EXP_SCATTER_STRIDED
    const int i_lo = wave_global, i_hi = count, i_step = U * wave_total, u_step = wave_total;
#else
    const int chunk = (count + wave_total - 1) / wave_total;
    const int i_lo = wave_global * chunk, i_hi = min(count, i_lo + chunk), i_step = U, u_step = 1;
#endif
#pragma unroll 1
    for (int i0 = i_lo; i0 < i_hi; i0 += i_step) {
        float4 q[U]; float gch[U]; bool on[U]; float o[U][6];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * u_step;
            on[u] = i < i_hi;
            const int n = __builtin_amdgcn_readfirstlane(a.list[on[u] ? i : i0]);
            q[u] = a.xw[n];
            if (CT == 24) gch[u] = a.gxpre[n];
            else gch[u] = (lane_on && on[u]) ? a.gg[(size_t)i * 48 + c0 + ch] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            Bl b[6];
            plane_setups(f, q[u].x, q[u].y, q[u].z, SCHED_TN(a), b);
            float val[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const bool my0 = dx0 ? b[p].m1 : b[p].m0, my1 = dx0 ? b[p].m3 : b[p].m2;
                const float wx = dx0 ? b[p].w : b[p].e;
                const size_t o0 = (size_t)(b[p].base + dx0) * CT + c0 + ch, o1 = o0 + (size_t)b[p].W * CT;
                const float v0 = (lane_on && my0) ? pl[p][o0] : 0.f, v1 = (lane_on && my1) ? pl[p][o1] : 0.f;
                const float part = v0 * (wx * b[p].s) + v1 * (wx * b[p].n);
                val[p] = part + dpp_xor1(part);
            }
            float L[6], Rr[6];
            L[0] = gch[u];
#pragma unroll
            for (int p = 1; p < 6; ++p) L[p] = L[p - 1] * val[p - 1];
            Rr[5] = 1.f;
#pragma unroll
            for (int p = 4; p >= 0; --p) Rr[p] = Rr[p + 1] * val[p + 1];
#pragma unroll
            for (int p = 0; p < 6; ++p) o[u][p] = L[p] * Rr[p];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!(lane_on && on[u])) continue;
            Bl b[6];
            plane_setups(f, q[u].x, q[u].y, q[u].z, SCHED_TN(a), b);
#pragma unroll
            for (int p = 0; p < 3; ++p) {       // space planes: coalesced global atomics
                if (!gp[p]) continue;
                const bool my0 = dx0 ? b[p].m1 : b[p].m0, my1 = dx0 ? b[p].m3 : b[p].m2;
                const float wx = dx0 ? b[p].w : b[p].e;
                const size_t o0 = (size_t)(b[p].base + dx0) * CT + c0 + ch, o1 = o0 + (size_t)b[p].W * CT;
                if (my0) atomicAdd(gp[p] + o0, (wx * b[p].s) * o[u][p]);
                if (my1) atomicAdd(gp[p] + o1, (wx * b[p].n) * o[u][p]);
            }
#pragma unroll
            for (int p = 3; p < 6; ++p) {       // time planes: workgroup-private LDS rows (y0, y0+1 are call constants)
                const bool my0 = dx0 ? b[p].m1 : b[p].m0, my1 = dx0 ? b[p].m3 : b[p].m2;
                const float wx = dx0 ? b[p].w : b[p].e;
                const int x = b[p].base - SCHED_Y0(a) * b[p].W + dx0;        // column inside the row
                float* r0 = acc_lds + ((size_t)((p - 3) * 2 + 0) * gmax + x) * 24 + ch;
                if (my0) atomicAdd(r0, (wx * b[p].s) * o[u][p]);
                if (my1) atomicAdd(r0 + (size_t)gmax * 24, (wx * b[p].n) * o[u][p]);
            }
        }
    }
    __syncthreads();
    // flush the private rows
    const int Gc[3] = {f.G[2], f.G[1], f.G[0]};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float* g = CT == 24 ? a.g.dpt[p] : a.g.apt[p];
        if (!g) continue;
        for (int dy = 0; dy < 2; ++dy) {
            const int y = SCHED_Y0(a) + dy;
            if (y < 0 || y >= f.K) continue;
            for (int k = threadIdx.x; k < Gc[p] * 24; k += blockDim.x) {
                const int x = k / 24, c = k - 24 * x;
                const float v = acc_lds[((size_t)(p * 2 + dy) * gmax + x) * 24 + c];
                if (v != 0.f) atomicAdd(g + ((size_t)y * Gc[p] + x) * CT + c0 + c, v);
            }
        }
    }
}

int64_t plane_elems(const nvfi_field_desc* f, int64_t* off /* [12]: dps[3] dpt[3] aps[3] apt[3] */) {
    const int A[3] = {0, 0, 1}, Bx[3] = {1, 2, 2}, Cc[3] = {2, 1, 0};
    int64_t n = 0;
    for (int i = 0; i < 3; ++i) { off[i] = n; n += (int64_t)f->G[A[i]] * f->G[Bx[i]] * f->Cd; }
    for (int i = 0; i < 3; ++i) { off[3 + i] = n; n += (int64_t)f->K * f->G[Cc[i]] * f->Cd; }
    for (int i = 0; i < 3; ++i) { off[6 + i] = n; n += (int64_t)f->G[A[i]] * f->G[Bx[i]] * f->Ca; }
    for (int i = 0; i < 3; ++i) { off[9 + i] = n; n += (int64_t)f->K * f->G[Cc[i]] * f->Ca; }
    return n;
}
int launch_scatter_det(ScatterArgs& sa, int C, int64_t N, hipStream_t st) {
    const unsigned sc_blocks = (unsigned)((N + 4 * SCATTER_SPW - 1) / (4 * SCATTER_SPW));
    if (C == 24) hipLaunchKernelGGL((k_plane_scatter<24, true>), dim3(sc_blocks), dim3(256), 0, st, sa);
    else hipLaunchKernelGGL((k_plane_scatter<48, true>), dim3(sc_blocks), dim3(256), 0, st, sa);
    LAUNCHCK();
    return 0;
}
int launch_det_finish(const nvfi_field_desc* f, const long long* shadow, const nvfi_grads* grads, hipStream_t st) {
    int64_t off[12];
    const int64_t total = plane_elems(f, off);
    float* const real[12] = {grads->dps[0], grads->dps[1], grads->dps[2], grads->dpt[0], grads->dpt[1], grads->dpt[2],
                             grads->aps[0], grads->aps[1], grads->aps[2], grads->apt[0], grads->apt[1], grads->apt[2]};
    for (int k = 0; k < 12; ++k) {
        if (!real[k]) continue;
        const int64_t n = (k + 1 < 12 ? off[k + 1] : total) - off[k];
        hipLaunchKernelGGL(k_det_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, shadow + off[k], real[k], n);
    }
    LAUNCHCK();
    return 0;
}
// plane-gradient scatter: LDS-privatised time rows when they fit, plain channel-parallel atomics otherwise
int launch_scatter(const nvfi_field_desc* f, ScatterArgs& sa, int C, int64_t N, float tn, hipStream_t st) {
    int gmax = f->G[0] > f->G[1] ? f->G[0] : f->G[1];
    gmax = gmax > f->G[2] ? gmax : f->G[2];
    const size_t lds = (size_t)6 * gmax * 24 * sizeof(float);
    if (lds <= 150 * 1024) {
        static DeviceOnce once;
        if (once.lds(152 * 1024, k_plane_scatter_lds<24>, k_plane_scatter_lds<48>)) return 1;
        sa.y0 = time_row0(*f, tn); sa.gmax = gmax;
        if (C == 24) hipLaunchKernelGGL(k_plane_scatter_lds<24>, dim3(256, 1), dim3(1024), lds, st, sa);
        else hipLaunchKernelGGL(k_plane_scatter_lds<48>, dim3(256, 2), dim3(1024), lds, st, sa);
    } else {
        const unsigned sc_blocks = (unsigned)((N + 4 * SCATTER_SPW - 1) / (4 * SCATTER_SPW));
        if (C == 24) hipLaunchKernelGGL(k_plane_scatter<24>, dim3(sc_blocks), dim3(256), 0, st, sa);
        else hipLaunchKernelGGL(k_plane_scatter<48>, dim3(sc_blocks), dim3(256), 0, st, sa);
    }
    LAUNCHCK();
    return 0;
}

