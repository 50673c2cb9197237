// reduce.h - the house rules of the loss and metric units (segloss.hip, metrics.hip, charloss.hip, depthloss.hip, raydist.hip, flowloss.hip) as code:
//   - every clear is a kernel (launch_zero or the unit's own), never a memset node;
//   - nothing waits for the device: every launch is on the caller's stream and the call can be captured in a hipGraph;
//   - no float atomic on a result: a value that is documented to repeat bit for bit is a plain store of a sum formed in a fixed order;
//   - partials are summed in fp64 in a fixed order - over the lanes by the butterfly below, over the waves and the workgroups in INDEX order -
//     so a result does not depend on which workgroup came last.
// In-launch hand-off ("the last workgroup finishes"): every workgroup publishes its partials, drains them and draws a ticket; the workgroup
// that draws the last ticket reads all partials back, in workgroup order.  Tickets are zero at launch.
// Not routed through here: regs.hip (another protocol: an ACQ_REL ticket from thread 0 over fp64 atomics into a slot ring) and the training
// step's kernels in render_rays.hip / scatter.hip / pde.hip, which write their hand-off inline.
#pragma once
#include "common.h"

// the butterfly of common.h's float wave_sum for NV values of fp64 or int, in place: the same order, every lane gets the same bits
template <int NV, class T> __device__ __forceinline__ void wave_sum_n(T* v) {
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
}
__device__ __forceinline__ double wave_sum(double v) { wave_sum_n<1>(&v); return v; }
__device__ __forceinline__ int wave_sum(int v) { wave_sum_n<1>(&v); return v; }

// relaxed agent-scope store / load of a partial: performed at the coherence point, not in a CU-local cache, so no fence is needed around them
#define RED_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
__device__ __forceinline__ void publish(float* p, float v) { __hip_atomic_store(p, v, RED_RLX); }
__device__ __forceinline__ float read_published(const float* p) { return __hip_atomic_load(p, RED_RLX); }
__device__ __forceinline__ void publish(double* p, double v) { __hip_atomic_store((long long*)p, __double_as_longlong(v), RED_RLX); }
__device__ __forceinline__ double read_published(const double* p) { return __longlong_as_double(__hip_atomic_load((const long long*)p, RED_RLX)); }

// every thread of the workgroup, after its publish calls: true in the workgroup that is the `total`-th to arrive at this ticket.  Every
// publishing wave drains its stores before the barrier, one lane then draws the ticket.
__device__ __forceinline__ bool last_arrival(int* ticket, int total) {
    __shared__ bool last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, RED_RLX) == total - 1;
    __syncthreads();
    return last;
}

// ordered sum of NV values per thread over a workgroup of NW waves (every thread calls it, with its lane and wave index): wave butterflies,
// then every thread adds the NW wave sums SEQUENTIALLY in wave-index order - all threads get the same bits.  part: NW * NV entries of LDS,
// reusable from call to call.
// (metrics.hip's met_block_sum and segloss.hip's seg_block_publish add four wave sums pairwise: other bits, their own lines.)
template <int NW, int NV, class T> __device__ __forceinline__ void block_sum_ordered(T* v, T* part, int lane, int wave) {
    wave_sum_n<NV>(v);
    __syncthreads();                                  // (the previous call's readers are done with `part`)
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NV; ++q) part[wave * NV + q] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        T s = 0;
        for (int w = 0; w < NW; ++w) s += part[w * NV + q];
        v[q] = s;
    }
}
