// pde.hip - velocity PDE regulariser: divergence + transport residual of the VelBasis field.
//
// Reference semantics: NVFi.get_vel_loss (models/nvfi.py:42-84):
//   occupancy prefilter (normalise, snap to keyframe, RK2 back-advect, density, alpha >= thres),
//   J = d(v,a)/d(x,y,z,t) of the un-gated vel_net (functorch vmap(jacrev)), div = tr J[:3,:3],
//   transport = J[:3,:3] v + J[:3,3] - a, loss = 5 mean(div^2) + 0.1 mean(transport^2),
//   and loss.backward() through the Jacobian (second order).
//
// MI355X design: the Jacobian is computed in FORWARD mode (value + 4 tangents pushed through the
// MFMA engine, all five columns of a 32-point tile in one workgroup: pde_jet.hip / pde_jet6.hip), the
// backward is the hand-written reverse of that tangent program (the four tangent adjoints feed their
// second-derivative corrections into the value adjoint in registers), fused by default with the hidden
// layers' weight gradients (pde_fuse.hip); the remaining weight gradients are split-K MFMA over the
// stashed tiles (launch_pde_wgrad below).  This unit holds the prefilter, the residuals and the host side.
// Points are bucketed by RK2 step count so workgroups of the prefilter are homogeneous.
#include <stddef.h>
#include <stdlib.h>
#include "common.h"
#include "vel.h"
#include "render.h"
#include "pde.h"
#include "fuse.h"
#include "scatter.h"
#include "frags.h"
#include "x6.h"

// ---------------------------------------------------------------- prefilter
__global__ __launch_bounds__(256) void k_pde_prep(PdePrepArgs a) {
    __shared__ int hist[PDE_MAX_CLASS];
    __shared__ int gbase[PDE_MAX_CLASS];
    if (threadIdx.x < PDE_MAX_CLASS) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool on = i < a.P;
    const nvfi_field_desc& f = a.f;
    int ns = 0, lr = 0;
    if (on) {
        const float t = a.t[i];
        const float base = snap_base(f, t);
        float xn[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xn[c] = norm_coord(f, c, a.points[3 * i + c]);
        a.qorig[i] = make_float4(xn[0], xn[1], xn[2], t);
        a.xw[i] = make_float4(xn[0], xn[1], xn[2], norm_time(f, base));
        // A point outside the velocity gate never moves (velocity_field.py:28-33,46-51: v = 0 there, so x_mid = x and the step leaves
        // x where it is - it stays outside for every later step): class 0, no network evaluations.  Exact, not an approximation.
        const bool frozen = gated_out(f, xn[0], xn[1], xn[2]);
        a.pt_t[i] = t; a.pt_base[i] = frozen ? t : base;
        // number of RK2 steps this point will take (same fp32 recurrence as the integrator)
        const float dtm = dt_max_of(f);
        float off = frozen ? 0.f : t - base;
        while (fabsf(off) > 0.f && ns < PDE_MAX_CLASS - 1) {
            float m = fminf(fabsf(off), dtm);
            off = off - (off > 0.f ? m : -m);
            ++ns;
        }
        a.cls[i] = ns;
        lr = atomicAdd(&hist[ns], 1);          // rank inside the workgroup (LDS atomic)
    }
    __syncthreads();
    if (threadIdx.x < PDE_MAX_CLASS && hist[threadIdx.x] > 0) gbase[threadIdx.x] = atomicAdd(&a.cls_count[threadIdx.x], hist[threadIdx.x]);
    __syncthreads();
    if (on) a.rank[i] = gbase[ns] + lr;
}
// bucket points by step count: perm[class_off[c] + rank] = i
__global__ __launch_bounds__(256) void k_pde_bucket(int64_t P, const int* cls, const int* rank, const int* cls_count, int* perm,
                                                    float* pt_t_perm, float* pt_base_perm, const float* pt_t, const float* pt_base) {
    __shared__ int off[PDE_MAX_CLASS];
    if (threadIdx.x == 0) {
        // most steps first: long-running workgroups start early
        int s = 0;
        for (int c = PDE_MAX_CLASS - 1; c >= 0; --c) { off[c] = s; s += cls_count[c]; }
    }
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int p = off[cls[i]] + rank[i];
    perm[p] = (int)i;
    pt_t_perm[p] = pt_t[i]; pt_base_perm[p] = pt_base[i];
}
// density at the warped point (k_density_q, scatter.hip) -> alpha -> keep flag (nvfi.py:56-64); one wave = 64 consecutive points
__global__ __launch_bounds__(256) void k_pde_keep(nvfi_field_desc f, int64_t P, const float* sig, uint8_t* flags, int* cnt) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < P) {
        const float alpha = 1.f - expf(-sig[i] * 0.01f * 25.f);
        keep = alpha >= f.alpha_thres;
        flags[i] = keep ? 1 : 0;
    }
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && i < P) cnt[i >> 6] = __popcll(b);
}

// k_pde_keep + the k_fill launch behind it (round 5): a wave = 64 consecutive points, a workgroup publishes its kept count and places its
// entries of the ordered kept list itself (look-back, common.h) - the list k_fill wrote, entry for entry
__global__ __launch_bounds__(256) void k_pde_keep_fill(nvfi_field_desc f, int64_t P, const float* sig, uint8_t* flags, unsigned long long* lb, int* klist, int* kcount) {
    __shared__ int ck[4];
    __shared__ unsigned long long excl_sh;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < P) {
        const float alpha = 1.f - expf(-sig[i] * 0.01f * 25.f);
        keep = alpha >= f.alpha_thres;
        flags[i] = keep ? 1 : 0;
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) ck[w] = __popcll(b);
    __syncthreads();
    if (w == 0) {
        const unsigned long long agg = (unsigned long long)((ck[0] + ck[1]) + (ck[2] + ck[3]));
        const unsigned long long e = lb_exclusive(lb, (int)blockIdx.x, agg);
        if (lane == 0) {
            excl_sh = e;
            if (blockIdx.x == gridDim.x - 1) *kcount = (int)(e + agg);
        }
    }
    __syncthreads();
    int base = (int)excl_sh;
    for (int k = 0; k < w; ++k) base += ck[k];
    if (keep) klist[base + __popcll(b & ((1ull << lane) - 1ull))] = (int)i;
}

// (The Jacobian passes - value + four tangent columns forward, their adjoints with the second-derivative corrections - live in pde_jet.hip,
// pde_jet6.hip and pde_fuse.hip; the column-parallel forms that stood here in rounds 1-5 were retired in round 6.)
// Round 5: the call's tiny bookkeeping kernels ride in k_pde_seeds.  Every workgroup of the launch draws a ticket when it is done (its
// partial sums are agent-scope atomics that have completed - s_waitcnt vmcnt(0) - before the ticket, as in k_tile_hist); the LAST one does the
// work of k_pde_pass_count (the sample count of this pass for the weight-gradient kernels, the fused adjoint's queue word), and - in the last
// pass of the call - of k_pde_finish (the value) and k_pde_counters.  One thread, a few dozen loads.
__device__ __forceinline__ void pde_tail(const PdeJetArgs& a, int count) {
    if (threadIdx.x != 0) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const PdeTail& T = a.tail;
    if (__hip_atomic_fetch_add(T.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (int)gridDim.x - 1) return;
    __hip_atomic_store(T.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (the next pass of the call draws from zero again)
    if (T.dcount) pde_write_pass_count(T.dcount, count);
    if (T.out)
        pde_write_finish(T.out, *a.kcount, __hip_atomic_load(a.sums + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                         __hip_atomic_load(a.sums + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (T.counters) pde_write_counters(T.counters, T.cls_count, a.kcount, T.P, T.pre16);
}
// K3: per-point residuals (nvfi.py:74-83), loss partial sums and adjoint seeds
__global__ __launch_bounds__(256) void k_pde_seeds(PdeJetArgs a) {
    __shared__ float red[8];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int count = pde_pass_count(a.kcount, a.first, a.cap);
    if ((int)(blockIdx.x * 256) >= count) { if (a.tail.ticket) pde_tail(a, count); return; }
    const bool active = i < count;
    const size_t cs = a.cap;
    const int capc = pde_group_ceil(count);   // the jet workgroups cover whole 128-point groups
    const float inv_n = 1.f / (float)(*a.kcount);
    float sd = 0.f, st = 0.f;
    if (i < capc) {
        float w[6], wd[4][6], aw[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            w[k] = a.wout[(size_t)k * cs + i]; aw[k] = a.wout[(size_t)(30 + k) * cs + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) wd[j][k] = a.wout[(size_t)(6 + 6 * j + k) * cs + i];
        }
        float4 q = active ? a.qorig[a.klist[a.first + i]] : zero4();
        const float x = q.x, y = q.y, z = q.z;
        float v[3], ac[3], Jv[3][4];
        vel_from_w(w, x, y, z, v);
        acc_from_w(aw, x, y, z, ac);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Jv[0][j] = wd[j][0] - wd[j][4] * z + wd[j][5] * y;
            Jv[1][j] = wd[j][1] + wd[j][3] * z - wd[j][5] * x;
            Jv[2][j] = wd[j][2] - wd[j][3] * y + wd[j][4] * x;
        }
        Jv[0][2] += -w[4]; Jv[0][1] += w[5];
        Jv[1][2] += w[3];  Jv[1][0] += -w[5];
        Jv[2][1] += -w[3]; Jv[2][0] += w[4];
        const float div = Jv[0][0] + Jv[1][1] + Jv[2][2];
        float tr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) tr[c] = Jv[c][0] * v[0] + Jv[c][1] * v[1] + Jv[c][2] * v[2] + Jv[c][3] - ac[c];
        float* sp = a.seeds + i;
        if (active) {
            sd = div * div; st = tr[0] * tr[0] + tr[1] * tr[1] + tr[2] * tr[2];
            const float lscale = a.scale_dev ? *a.scale_dev : a.scale;
            const float gdiv = lscale * 10.f * div * inv_n;
            float gtr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) gtr[c] = lscale * 0.2f * tr[c] * inv_n / 3.f;
            float gJ[3][4], gv[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { gJ[c][k] = gtr[c] * v[k]; gv[k] += gtr[c] * Jv[c][k]; }
                gJ[c][3] = gtr[c];
                gJ[c][c] += gdiv;
            }
            sp[0 * cs] = gv[0]; sp[1 * cs] = gv[1]; sp[2 * cs] = gv[2];
            sp[3 * cs] = z * gv[1] - y * gv[2] + gJ[1][2] - gJ[2][1];
            sp[4 * cs] = -z * gv[0] + x * gv[2] - gJ[0][2] + gJ[2][0];
            sp[5 * cs] = y * gv[0] - x * gv[1] + gJ[0][1] - gJ[1][0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sp[(6 + 6 * j + 0) * cs] = gJ[0][j]; sp[(6 + 6 * j + 1) * cs] = gJ[1][j]; sp[(6 + 6 * j + 2) * cs] = gJ[2][j];
                sp[(6 + 6 * j + 3) * cs] = z * gJ[1][j] - y * gJ[2][j];
                sp[(6 + 6 * j + 4) * cs] = -z * gJ[0][j] + x * gJ[2][j];
                sp[(6 + 6 * j + 5) * cs] = y * gJ[0][j] - x * gJ[1][j];
            }
            const float ga[3] = {-gtr[0], -gtr[1], -gtr[2]};
            sp[30 * cs] = ga[0]; sp[31 * cs] = ga[1]; sp[32 * cs] = ga[2];
            sp[33 * cs] = -y * ga[1] - z * ga[2];
            sp[34 * cs] = -x * ga[0] - z * ga[2];
            sp[35 * cs] = -x * ga[0] - y * ga[1];
            if (a.jac && (a.first + i) < a.n_jac) {
                float* jp = a.jac + (size_t)(a.first + i) * 24;
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) jp[c * 4 + j] = Jv[c][j];
#pragma unroll
                for (int k = 12; k < 24; ++k) jp[k] = 0.f;
            }
        } else {
            // ragged tail of the last workgroup: zero seeds so that every adjoint stash row is zero
            for (int k = 0; k < 36; ++k) sp[(size_t)k * cs] = 0.f;
        }
    }
    sd = wave_sum(sd); st = wave_sum(st);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sd; red[4 + (threadIdx.x >> 6)] = st; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(a.sums + 0, (double)(red[0] + red[1] + red[2] + red[3]));
        atomicAdd(a.sums + 1, (double)(red[4] + red[5] + red[6] + red[7]));
    }
    if (a.tail.ticket) pde_tail(a, count);
}

// the same bookkeeping as launches of their own (NVFI_FUSED_LAUNCH=0): no synchronisation on the launch stream.  The writers are pde.h's
__global__ void k_pde_pass_count(const int* kcount, int64_t first, int64_t cap, int* dcount) {
    if (threadIdx.x == 0) pde_write_pass_count(dcount, pde_pass_count(kcount, first, cap));
}
__global__ void k_pde_counters(const int* cls_count, const int* kcount, int64_t P, int pre16, int64_t* c8) {
    if (threadIdx.x == 0) pde_write_counters(c8, cls_count, kcount, P, pre16);
}
__global__ void k_pde_finish(const double* sums, const int* kcount, float* out) {
    if (threadIdx.x == 0) pde_write_finish(out, *kcount, sums[0], sums[1]);
}

// ---------------------------------------------------------------- host
struct PdePlan {
    float4 *qorig, *xw;
    float *pt_t, *pt_base, *pt_t_perm, *pt_base_perm;
    int *cls, *rank, *cls_count, *perm, *cnt, *off, *klist, *kcount, *dcount;
    uint8_t* flags;
    float* sig;     // density at the warped points (prefilter)
    float4* xw16; uint8_t* near; int* blist; int* bcount; void* img16; void* img16lo;   // fp16 pre-pass (pre16.hip)
    void* x6img;                                                                       // x6 prefilter (vel_x6.hip)
    double* sums; unsigned long long* lb; int64_t zero_bytes;
    float *vel_frag, *a_frag, *vel_x4f, *vel_x4b, *a_x4b, *stash, *seeds, *wout, *slabs;
    int64_t chunk, total;
};
// the block one fill clears at the start of a call: the class histogram + counts (PDE_MAX_CLASS + 16 ints: [+0] kept, [+1] band, [+2] ticket of
// k_pde_seeds' tail), the four double loss sums and the look-back words of k_pde_keep_fill (one per workgroup of 256 points)
struct PdeZeroed { int cls_count[PDE_MAX_CLASS + 16]; double sums[4]; unsigned long long lb[1]; };
static void plan_pde(int64_t P, void* ws, PdePlan* L) {
    Bump B{(char*)ws, 0, 0};
    const int64_t nw = (P + 63) / 64;
    L->qorig = B.take<float4>(P); L->xw = B.take<float4>(P);
    L->pt_t = B.take<float>(P); L->pt_base = B.take<float>(P); L->pt_t_perm = B.take<float>(P); L->pt_base_perm = B.take<float>(P);
    L->cls = B.take<int>(P); L->rank = B.take<int>(P);
    L->zero_bytes = (int64_t)offsetof(PdeZeroed, lb) + ((P + 255) / 256) * (int64_t)sizeof(unsigned long long);
    char* z = B.take<char>(L->zero_bytes);
    L->cls_count = reinterpret_cast<int*>(z + offsetof(PdeZeroed, cls_count)); L->sums = reinterpret_cast<double*>(z + offsetof(PdeZeroed, sums));
    L->lb = reinterpret_cast<unsigned long long*>(z + offsetof(PdeZeroed, lb));
    L->kcount = L->cls_count + PDE_MAX_CLASS; L->bcount = L->cls_count + PDE_MAX_CLASS + 1;
    L->perm = B.take<int>(P);
    L->cnt = B.take<int>(nw); L->off = B.take<int>(nw + 1); L->klist = B.take<int>(P);
    L->flags = B.take<uint8_t>(nw * 64);
    L->sig = B.take<float>(nw * 64);
    L->xw16 = B.take<float4>(P); L->near = B.take<uint8_t>(nw * 64); L->blist = B.take<int>(P);
    L->img16 = B.take<float4>(PRE16_IMAGE_BYTES / 16);
    L->img16lo = B.take<float4>(PRE16_IMAGE_BYTES / 16);
    L->x6img = B.take<float4>(X6_IMAGE_BYTES / 16);
    L->dcount = B.take<int>(16);
    L->vel_frag = B.take<float>(VEL_FRAG_FLOATS); L->a_frag = B.take<float>(VEL_FRAG_FLOATS);
    L->vel_x4f = B.take<float>(VEL_X4F_FLOATS); L->vel_x4b = B.take<float>(VEL_X4B_FLOATS);      // (with T0, which no PDE kernel reads: the set travels whole)
    L->a_x4b = B.take<float>(A_X4B_FLOATS);                                                      // transposed fragments of a_weight_net (pde_fuse.hip)
    L->chunk = P < PDE_CHUNK ? pde_group_ceil(P) : PDE_CHUNK;
    L->stash = B.take<float>(L->chunk / TILE * (int64_t)PDE_TILE_ROWS * REGF);
    L->seeds = B.take<float>(36 * L->chunk);
    L->wout = B.take<float>(36 * L->chunk);
    L->slabs = B.take<float>((int64_t)PDE_NSLAB * (128 * 128 + 128) * 18);
    L->total = align_up(B.off, 256);
}
extern "C" int nvfi_pde_workspace_bytes(const nvfi_field_desc* f, int64_t P, int64_t* bytes) {
    (void)f;
    PdePlan L; plan_pde(P, nullptr, &L);
    *bytes = L.total;
    return 0;
}

// A call, resolved once: what the caller passed ...
struct PdeCall {
    const nvfi_field_desc* f; int64_t P; const float* points; const float* t;
    float scale; const float* scale_dev;       // loss scale by value, or (non-NULL) read from device memory (nvfi_pde_loss_dev)
    float* out; const nvfi_grads* grads; void* workspace; int64_t workspace_bytes; int64_t* counters;
    uint8_t* kept_out; float* jac; int64_t n_jac; int64_t* host_info;
    hipStream_t st;
    hipStream_t bwd;        // nvfi_pde_loss_split: the stream of the adjoint + weight-gradient half (NULL: everything on st)
};
// ... and what the switches (switches.h) say
struct PdeModes {
    // prefilter: x6 (default, round 5: vel_x6.hip - the fp32 products of the hidden layers formed exactly on the 16-bit matrix pipe, from three
    // binary16 terms per operand: its error against float64 is not larger than the fp32 MFMA kernel's, tests/test_gpu_x6.py, and it is 1.35x
    // faster) | fp32 (the feature-split fp32 MFMA kernel of vel_split.hip, the default of rounds 2-4; "split32" = "fp32"; "engine32", k_rk2_fwd of
    // vel.hip with the same numbers bit for bit and ~4 % slower, was retired in round 6) | fp16band (pre16.hip: fp16-input pass + fp32
    // re-evaluation of the unsafe points) | split16band (opt-in, pre16.hip: the pre-pass with fp32 products emulated by two binary16 terms per
    // operand - three fp16 MFMAs - and a band 100 x narrower than fp16band's in front of the same fp32 re-evaluation)
    int prefilter;
    float band, eps_gate;       // the band modes' alpha band and gate margin
    bool fused_launch;          // NVFI_FUSED_LAUNCH: k_pde_keep_fill, and the bookkeeping in k_pde_seeds' last workgroup
    // NVFI_PDE_FUSE (default 1): pde_fuse.hip - weight_net's Jacobian adjoint and its four 128 x 128 weight gradients in one persistent kernel
    // (no gz_1..gz_4 stash, no second pass over the z / zd stash); 0: k_pde_jet_bwd + k_wgrad_ring8 over the full adjoint stash
    bool fuse;
    bool jet_x6;                // NVFI_PDE_JET_X6 (default 1, round 6): pde_jet6.hip - the Jacobian forward with the hidden layers on the 16-bit matrix pipe
    bool deterministic;         // NVFI_DETERMINISTIC: the fused adjoint's second half takes a static share of tiles instead of its queue
    bool band_mode() const { return prefilter == PRE_FP16BAND || prefilter == PRE_SPLIT16BAND; }
};
static int pde_modes(PdeModes* m) {
    m->prefilter = sw(NVFI_PDE_PREFILTER);
    if (m->prefilter == PRE_UNKNOWN) return nvfi_fail(2, "NVFI_PDE_PREFILTER must be fp32, x6, fp16band or split16band");
    const bool narrow = m->prefilter == PRE_SPLIT16BAND;
    m->band = narrow ? 1e-3f : 0.1f; m->eps_gate = narrow ? 2e-5f : 2e-3f;
    m->fused_launch = sw(NVFI_FUSED_LAUNCH) != 0; m->fuse = sw(NVFI_PDE_FUSE) != 0;
    m->jet_x6 = sw(NVFI_PDE_JET_X6) != 0; m->deterministic = sw(NVFI_DETERMINISTIC) != 0;
    return 0;
}
// the fused adjoint is the only reader of the hidden layers' pre-activations as x4 stash blocks: it runs when all four hidden-layer gradients of
// weight_net are wanted
static bool pde_fuse_ok(const PdeCall& c, const PdeModes& m) {
    const nvfi_grads* g = c.grads;
    return m.fuse && g && g->vW[1] && g->vW[2] && g->vW[3] && g->vW[4];
}

// ---- stage 1: the occupancy prefilter.  Step classes and bucket order, RK2 back-advection in bucket order (per-point times), density
static int pde_density(const PdeCall& c, const PdePlan& L, const float4* xw, const int* count, const int* list) {
    DensityArgs da; memset(&da, 0, sizeof(da));
    da.f = *c.f; da.per_point_t = 1; da.sigma_out = L.sig; da.n_direct = c.P; da.xw = xw; da.count = count; da.list = list;
    return launch_density_q(da, c.P, c.st);
}
// the per-point arguments every warp launcher takes (SplitArgs, X6Args, Pre16Args name them alike)
struct PdeWarpPoints { const int* list; float4* xw; const float* pt_t; const float* pt_base; float dt_max; int max_steps; };
template <class A> static A pde_warp_args(const PdeCall& c, const PdeWarpPoints& p) {
    A a; memset(&a, 0, sizeof(a));
    a.f = *c.f; a.list = p.list; a.xw = p.xw; a.pt_t = p.pt_t; a.pt_base = p.pt_base; a.dt_max = p.dt_max; a.max_steps = p.max_steps;
    return a;
}
static SplitArgs pde_split_args(const PdeCall& c, const PdeWarpPoints& p, const VelImages& VI) {
    SplitArgs sa = pde_warp_args<SplitArgs>(c, p);
    for (int l = 0; l < 6; ++l) { sa.f4[l] = VI.f4[l]; sa.bv[l] = VI.VW.b[l]; }
    return sa;
}
static int pde_prefilter(const PdeCall& c, const PdeModes& m, const PdePlan& L, const VelImages& VI) {
    const int64_t P = c.P;
    const unsigned pb = (unsigned)((P + 255) / 256);
    PdePrepArgs pa; pa.f = *c.f; pa.P = P; pa.points = c.points; pa.t = c.t; pa.qorig = L.qorig; pa.xw = L.xw; pa.pt_t = L.pt_t; pa.pt_base = L.pt_base;
    pa.cls = L.cls; pa.rank = L.rank; pa.cls_count = L.cls_count;
    hipLaunchKernelGGL(k_pde_prep, dim3(pb), dim3(256), 0, c.st, pa);
    hipLaunchKernelGGL(k_pde_bucket, dim3(pb), dim3(256), 0, c.st, P, L.cls, L.rank, L.cls_count, L.perm, L.pt_t_perm, L.pt_base_perm, L.pt_t, L.pt_base);
    LAUNCHCK();
    const PdeWarpPoints bucketed = {L.perm, L.xw, L.pt_t_perm, L.pt_base_perm, dt_max_of(*c.f), PDE_MAX_CLASS};
    if (m.prefilter == PRE_FP32) {
        SplitArgs sa = pde_split_args(c, bucketed, VI);
        sa.n_direct = P;
        if (launch_rk2_split(sa, P, c.st)) return 1;
        return pde_density(c, L, L.xw, nullptr, nullptr);
    }
    if (m.prefilter == PRE_X6) {
        X6Args xa = pde_warp_args<X6Args>(c, bucketed);
        xa.img = VI.x6; xa.n_direct = P;
        { ProfScope ps(PK_PDE_PREFILTER, c.st); if (launch_rk2_x6(xa, P, c.st)) return 1; }
        return pde_density(c, L, L.xw, nullptr, nullptr);
    }
    // opt-in (pre16.hip): fp16-input pass over every candidate, then the fp32 kernel for the points whose decision is not safe
    Pre16Args qa = pde_warp_args<Pre16Args>(c, bucketed);
    qa.img = L.img16; qa.img_lo = m.prefilter == PRE_SPLIT16BAND ? L.img16lo : nullptr; qa.P = P; qa.xout = L.xw16; qa.near = L.near; qa.eps_gate = m.eps_gate;
    if (launch_pre16(c.f, qa, c.st)) return 1;
    if (pde_density(c, L, L.xw16, nullptr, nullptr)) return 1;
    if (launch_pde_band(c.f, P, L.perm, L.sig, L.near, m.band, L.flags, L.cnt, c.st)) return 1;
    launch_scan_fill(L.cnt, L.off, (P + 63) / 64, L.bcount, L.flags, L.blist, c.st);
    if (launch_pde_band_map(P, L.bcount, L.perm, L.blist, c.st)) return 1;
    // short list, long trajectories: the feature-split kernel (a tile's latency, not the chip's throughput, bounds this pass)
    SplitArgs sa = pde_split_args(c, PdeWarpPoints{L.blist, L.xw, L.pt_t, L.pt_base, bucketed.dt_max, PDE_MAX_CLASS}, VI);
    sa.count = L.bcount; sa.pt_by_list = 1;
    if (launch_rk2_split(sa, P, c.st)) return 1;
    return pde_density(c, L, L.xw, L.bcount, L.blist);
}

// ---- stage 2: alpha -> keep flags -> the ordered kept list and its device-side count
static int pde_keep(const PdeCall& c, const PdeModes& m, const PdePlan& L) {
    const unsigned pb = (unsigned)((c.P + 255) / 256);
    if (m.fused_launch) hipLaunchKernelGGL(k_pde_keep_fill, dim3(pb), dim3(256), 0, c.st, *c.f, c.P, L.sig, L.flags, L.lb, L.klist, L.kcount);
    else {
        hipLaunchKernelGGL(k_pde_keep, dim3(pb), dim3(256), 0, c.st, *c.f, c.P, L.sig, L.flags, L.cnt);
        launch_scan_fill(L.cnt, L.off, (c.P + 63) / 64, L.kcount, L.flags, L.klist, c.st);
    }
    LAUNCHCK();
    return 0;
}

// ---- host_info.  The kept count stays on the device (L.kcount): the jet passes are launched with worst-case grids and size themselves from it.
// Only a caller that asks for host_info (diagnostics; the Python mirror's `return 0.` decision, nvfi.py:66) pays a synchronisation: HOST_READ
// copies the counts and waits right behind the prefilter.  A split call (nvfi_pde_loss_split: the reference's loop) waits LATER - HOST_QUEUE
// once the Jacobian forward and the value are queued on `stream`, HOST_WAIT once the adjoint half is queued on the other one: the host's wait then
// covers the prefilter AND the forward (the caller's own wait for the value, `if loss_vel > 0`, returns at once) and the device does not idle
// between the prefilter and the jets while the host wakes up (30-140 us per iteration in a trace).
enum PdeHostStep { HOST_READ, HOST_QUEUE, HOST_WAIT };
static int pde_host_info(const PdeCall& c, const PdePlan& L, PdeHostStep step) {
    // (static storage, per host thread: an error return between the copy being queued and the wait must not leave the copy a dead stack frame
    // to write into - ADVICE r4)
    static thread_local int hcnt[PDE_MAX_CLASS + 16];
    if (step != HOST_WAIT) HIPCK(hipMemcpyAsync(hcnt, L.cls_count, sizeof(hcnt), hipMemcpyDeviceToHost, c.st));
    if (step == HOST_QUEUE) return 0;
    HIPCK(hipStreamSynchronize(c.st));
    int64_t evals = 0;
    for (int k = 0; k < PDE_MAX_CLASS; ++k) evals += 2ll * k * hcnt[k];
    c.host_info[0] = hcnt[PDE_MAX_CLASS]; c.host_info[1] = evals;
    return 0;
}

// ---- stage 3, per chunk of kept points [first, first + cap): the Jacobian forward, the residuals and the adjoint seeds
static int pde_forward(const PdeCall& c, const PdeModes& m, const PdePlan& L, const VelImages& VI, int64_t first, PdeJetArgs* chunk) {
    const int64_t cap = c.P - first < L.chunk ? pde_group_ceil(c.P - first) : L.chunk;
    PdeJetArgs& ja = *chunk; memset(&ja, 0, sizeof(ja));
    ja.Wv = VI.VW; ja.Wa = VI.AW; ja.qorig = L.qorig; ja.klist = L.klist; ja.first = first; ja.kcount = L.kcount; ja.cap = cap; ja.wgs = (int)(cap / WG_SAMPLES);
    ja.stash = L.stash; ja.seeds = L.seeds; ja.wout = L.wout; ja.sums = L.sums; ja.scale = c.scale; ja.scale_dev = c.scale_dev; ja.jac = c.jac; ja.n_jac = c.n_jac;
    for (int l = 0; l < 6; ++l) { ja.f4[l] = VI.f4[l]; ja.t4[l] = VI.t4[l]; ja.bv[l] = VI.VW.b[l]; }
    // the fused adjoint is the only reader of the hidden layers' pre-activations: they travel as x4 stash blocks (row-major for the unfused adjoint)
    ja.x4 = pde_fuse_ok(c, m) ? 1 : 0;
    ProfScope ps(PK_PDE_FWD, c.st);
    // all five weight_net columns of a tile in one workgroup; the ReLU acceleration net keeps its column kernel
    // (the launch carries the acceleration net's value column as trailing workgroups: they fill the tail of the jet tiles)
    if (m.jet_x6) {
        if (launch_pde_jet6_fwd(ja, VI.x6, (unsigned)(cap / TILE), (unsigned)ja.wgs, c.st)) return 1;
    } else if (launch_pde_jet_fwd(ja, (unsigned)(cap / TILE), (unsigned)ja.wgs, c.st)) return 1;
    if (m.fused_launch) {
        // the last workgroup of k_pde_seeds does the bookkeeping launches' work (pde_tail); out / counters in the last pass of the call only
        const bool last_pass = first + L.chunk >= c.P;
        ja.tail.ticket = L.cls_count + PDE_MAX_CLASS + 2; ja.tail.dcount = c.grads ? L.dcount : nullptr;
        ja.tail.out = last_pass ? c.out : nullptr;
        ja.tail.counters = last_pass ? c.counters : nullptr; ja.tail.cls_count = L.cls_count; ja.tail.P = c.P; ja.tail.pre16 = m.band_mode() ? 1 : 0;
    }
    hipLaunchKernelGGL(k_pde_seeds, dim3((unsigned)(cap / 256 + 1)), dim3(256), 0, c.st, ja);
    return 0;
}

// ---- stage 4, per chunk: the adjoint and the weight gradients
// a split call: the value is finished on st first, the adjoint half follows on the other stream behind an event (one per device, as render.hip's)
static PerDevice<hipEvent_t> g_split_ev;
static int pde_fork(const PdeCall& c, const PdeModes& m, const PdePlan& L) {
    hipEvent_t* ev = g_split_ev.get([](hipEvent_t& e, int) { HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return 0; });
    if (!ev) return 1;
    if (!m.fused_launch) hipLaunchKernelGGL(k_pde_finish, dim3(1), dim3(64), 0, c.st, L.sums, L.kcount, c.out);
    // the host's copy of the counts is queued IN FRONT of the adjoint half: k_pde_fuse_bwd owns every CU for ~0.4 ms (12 waves x 168
    // registers, 152 KB of LDS per workgroup) and a copy kernel queued behind its start waits for its first workgroup to retire - the
    // caller's `if loss_vel > 0` then returned 0.43 ms late (trace of the drop-in loop)
    if (c.host_info && pde_host_info(c, L, HOST_QUEUE)) return 1;
    HIPCK(hipEventRecord(*ev, c.st));
    HIPCK(hipStreamWaitEvent(c.bwd, *ev, 0));
    return 0;
}
// pde_fuse.hip: the adjoint of weight_net's five columns AND its four hidden-layer weight gradients in one persistent kernel
static int pde_fused_adjoint(const PdeCall& c, const PdeModes& m, const PdePlan& L, const VelImages& VI, const PdeJetArgs& ja, hipStream_t sb,
                             float* slabs, float* slabs_a, int* nslab, int* accel) {
    PdeFuseArgs fa; memset(&fa, 0, sizeof(fa));
    for (int l = 0; l < 6; ++l) { fa.t4[l] = VI.t4[l]; fa.ta4[l] = VI.ta4[l]; }
    fa.kcount = L.kcount; fa.first = ja.first; fa.cap = ja.cap; fa.stash = L.stash; fa.seeds = L.seeds; fa.x4 = ja.x4;
    fa.slabs = slabs; fa.layer_stride = (int64_t)PDE_NSLAB * (128 * 128 + 128); fa.slab_floats = 128 * 128 + 128;
    // ... and, when all four hidden-layer gradients of a_weight_net are wanted, its adjoint + those gradients as the kernel's second
    // half (tiles from a device-side queue); otherwise the acceleration net's adjoint keeps k_pde_jet_bwd's trailing workgroups
    // (a launch with zero jet tiles)
    const nvfi_grads* g = c.grads;
    fa.do_accel = (g->aW[1] && g->aW[2] && g->aW[3] && g->aW[4]) ? 1 : 0;
    fa.slabs_a = slabs_a;
    fa.queue = m.deterministic ? nullptr : L.dcount + 8;
    if (!fa.do_accel && launch_pde_jet_bwd(ja, 0, (unsigned)ja.wgs, sb)) return 1;
    // a split call (the reference's loop: the caller waits for the value - `if loss_vel > 0` - while this half runs on the other
    // stream) leaves 8 CUs to the caller's comparison / copy kernels: a persistent workgroup owns its CU, and behind 256 of them
    // that wait was 0.35 ms
    const int max_wgs = sb != c.st ? PDE_NSLAB - 8 : PDE_NSLAB;
    *accel = fa.do_accel;
    return launch_pde_fuse_bwd(fa, ja.cap, max_wgs, nslab, sb);
}
static int pde_adjoint(const PdeCall& c, const PdeModes& m, const PdePlan& L, const VelImages& VI, const PdeJetArgs& ja, bool split) {
    if (split && pde_fork(c, m, L)) return 1;
    const hipStream_t sb = split ? c.bwd : c.st;
    int fused_nslab = 0, fused_accel = 0;
    float* fused_slabs = L.slabs + (size_t)14 * PDE_NSLAB * (128 * 128 + 128);      // sets 14..17 (launch_pde_wgrad uses at most 10 beside them)
    float* fused_slabs_a = L.slabs + (size_t)10 * PDE_NSLAB * (128 * 128 + 128);    // sets 10..13 (at most 6 ring jobs are left then)
    // (before the adjoint: the fused kernel's queue word is cleared by the same launch)
    if (!m.fused_launch) hipLaunchKernelGGL(k_pde_pass_count, dim3(1), dim3(64), 0, sb, L.kcount, ja.first, ja.cap, L.dcount);
    {
        ProfScope ps(PK_PDE_BWD, sb);
        if (ja.x4) {
            if (pde_fused_adjoint(c, m, L, VI, ja, sb, fused_slabs, fused_slabs_a, &fused_nslab, &fused_accel)) return 1;
        } else if (launch_pde_jet_bwd(ja, (unsigned)(ja.cap / TILE), (unsigned)ja.wgs, sb)) return 1;
    }
    LAUNCHCK();
    if (launch_pde_wgrad(L.stash, (int)(ja.cap / TILE), L.slabs, L.dcount, c.grads, sb, fused_nslab, fused_slabs, fused_accel ? fused_slabs_a : nullptr)) return 1;
    return (split && c.host_info) ? pde_host_info(c, L, HOST_WAIT) : 0;
}

static int pde_loss_run(const PdeCall& c) {
    const int64_t P = c.P;
    if (P <= 0) return nvfi_fail(2, "P must be positive");
    if (P >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "P too large");
    if (!c.f->use_vel) return nvfi_fail(2, "PDE loss needs use_vel");
    if (ensure_lds_attrs()) return 1;
    PdePlan L; plan_pde(P, c.workspace, &L);
    if (L.total > c.workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld bytes, got %lld", (long long)L.total, (long long)c.workspace_bytes);
    if (launch_zero(L.cls_count, L.zero_bytes, c.st)) return 1;     // histogram / counts, loss sums, look-back words: one fill (a kernel, not hipMemsetAsync: common.h)
    PdeModes m;
    if (int rc = pde_modes(&m)) return rc;
    // the velocity net's images (frags.h): the cache's, or packed here - one k_pack, one k_frag_x4 per net, one x6 pack
    // (the jet kernels read x4 copies of the v-net fragments)
    const unsigned need = VI_VEL | VI_ANET | VI_X4F | VI_X4B | ((m.fuse && c.grads) ? VI_A_X4B : 0) | ((m.prefilter == PRE_X6 || m.jet_x6) ? VI_X6 : 0);
    VelImages VI;
    if (int rc = vel_images(c.f, need, VelImageRoom{L.vel_frag, L.a_frag, L.vel_x4f, L.vel_x4b, L.a_x4b, L.x6img, nullptr}, &VI, nullptr, 0, c.st)) return rc;
    if (pde_prefilter(c, m, L, VI) || pde_keep(c, m, L)) return 1;
    // the adjoint half of a split call runs on the other stream; a candidate count above one chunk falls back to one stream (the chunks share the stash)
    const bool split = c.grads && c.bwd && P <= L.chunk;
    if (c.host_info && !split && pde_host_info(c, L, HOST_READ)) return 1;
    if (c.kept_out) HIPCK(hipMemcpyAsync(c.kept_out, L.flags, (size_t)P, hipMemcpyDeviceToDevice, c.st));
    for (int64_t first = 0; first < P; first += L.chunk) {
        PdeJetArgs chunk;
        if (pde_forward(c, m, L, VI, first, &chunk)) return 1;
        if (c.grads && pde_adjoint(c, m, L, VI, chunk, split)) return 1;
        LAUNCHCK();
    }
    // NVFI_FUSED_LAUNCH=0: the value (a split call's was finished in front of its fork) and the counters as launches of their own
    if (!m.fused_launch) {
        if (!split) hipLaunchKernelGGL(k_pde_finish, dim3(1), dim3(64), 0, c.st, L.sums, L.kcount, c.out);
        if (c.counters) hipLaunchKernelGGL(k_pde_counters, dim3(1), dim3(64), 0, c.st, L.cls_count, L.kcount, P, m.band_mode() ? 1 : 0, c.counters);
        LAUNCHCK();
    }
    return 0;
}

extern "C" int nvfi_pde_loss_ex(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, float loss_scale,
                                float* out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters,
                                uint8_t* kept_out, float* jac_out, int64_t n_jac, int64_t* host_info, void* stream) {
    return pde_loss_run(PdeCall{f, P, points, t, loss_scale, nullptr, out, grads, workspace, workspace_bytes, counters, kept_out, jac_out, n_jac, host_info,
                                (hipStream_t)stream, nullptr});
}

/* The VALUE of the loss (out[]) is complete on `stream` after the Jacobian forward; the adjoint pass and the weight gradients - a third of the
 * call's time, needed only by the caller's backward - run on `bwd_stream`, ordered behind the forward by an event.  For a caller that waits
 * for the value on `stream` right after the call (train_nvfi.py:233 `if loss_vel > 0`) and then issues other work there (the renders'
 * backward), the two overlap.  The caller orders its use of the gradients (and the release of the workspace) behind `bwd_stream`.
 * A candidate count above one chunk (262 144) falls back to one stream: the chunks share the stash. */
extern "C" int nvfi_pde_loss_split(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, float loss_scale,
                                   float* out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters,
                                   uint8_t* kept_out, float* jac_out, int64_t n_jac, int64_t* host_info, void* stream, void* bwd_stream) {
    return pde_loss_run(PdeCall{f, P, points, t, loss_scale, nullptr, out, grads, workspace, workspace_bytes, counters, kept_out, jac_out, n_jac, host_info,
                                (hipStream_t)stream, bwd_stream != stream ? (hipStream_t)bwd_stream : nullptr});
}

extern "C" int nvfi_pde_loss_dev(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, const float* loss_scale_dev,
                                 float* out, const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream) {
    if (!loss_scale_dev) return nvfi_fail(2, "nvfi_pde_loss_dev: loss_scale_dev is NULL");
    return pde_loss_run(PdeCall{f, P, points, t, 1.f, loss_scale_dev, out, grads, workspace, workspace_bytes, counters, nullptr, nullptr, 0, nullptr,
                                (hipStream_t)stream, nullptr});
}

extern "C" int nvfi_pde_loss(const nvfi_field_desc* f, int64_t P, const float* points, const float* t, float loss_scale, float* out,
                             const nvfi_grads* grads, void* workspace, int64_t workspace_bytes, int64_t* counters, void* stream) {
    return nvfi_pde_loss_ex(f, P, points, t, loss_scale, out, grads, workspace, workspace_bytes, counters, nullptr, nullptr, 0, nullptr, stream);
}

// weight gradients of both nets from one chunk's stash
// fused_nslab > 0: the slabs of weight_net's four hidden layers were already written (fused_nslab of them each, value + tangent columns
// summed) by k_pde_fuse_bwd - only its two edge layers and the acceleration net are contracted here, the reduce covers everything
// (fused_slabs_a: likewise for a_weight_net, when the kernel's second half ran)
int launch_pde_wgrad(const float* stash, int ntiles, float* slabs, int* dcount, const nvfi_grads* G, hipStream_t st, int fused_nslab, const float* fused_slabs,
                     const float* fused_slabs_a) {
    const size_t ts = (size_t)PDE_TILE_ROWS * REGF;
    const size_t slab = (size_t)PDE_NSLAB * (128 * 128 + 128);
    // k_wgrad reads the sample count from device memory (dcount, set by k_pde_pass_count: no host sync); ntiles is the capacity
    WgradJobs wj; wj.n = 0; ReduceJobs rj; rj.n = 0;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < 6; ++l) {
            float* gW = net == 0 ? G->vW[l] : G->aW[l];
            float* gb = net == 0 ? G->vb[l] : G->ab[l];
            if (!gW && !gb) continue;
            if (fused_nslab > 0 && l >= 1 && l <= 4 && (net == 0 || fused_slabs_a)) {
                ReduceJob& Q = rj.j[rj.n++];
                memset(&Q, 0, sizeof(Q));
                Q.slabs = (net == 0 ? fused_slabs : fused_slabs_a) + (size_t)(l - 1) * slab; Q.nslab = fused_nslab; Q.MTA = 4; Q.KTB = 4; Q.gW = gW; Q.gb = gb;
                Q.out = 128; Q.in = 128; Q.row_kind = RK_NATURAL; Q.slot_kind = SK_HIDDEN; Q.scale = 1.f;
                continue;
            }
            const int npass = net == 0 ? 2 : 1;    // weight_net: value column + 4 tangent columns
            float* sl[2] = {nullptr, nullptr};
            for (int pass = 0; pass < npass; ++pass) {
                WgradJob& J = wj.j[wj.n];
                memset(&J, 0, sizeof(J));
                J.a_tile_stride = ts; J.b_tile_stride = ts; J.a_regs = l < 5 ? 64 : 16; J.count = dcount; J.cap_tiles = ntiles;
                J.slabs = slabs + (size_t)wj.n * slab; J.nslab = PDE_NSLAB;
                sl[pass] = J.slabs;
                ++wj.n;
                if (pass == 0) {              // value column: a_weight_net (ReLU) | weight_net (SiLU)
                    const int ga = net == 1 ? PDE_GAA : PDE_GA, z = net == 1 ? PDE_ZA : PDE_Z;
                    J.A = stash + (size_t)(ga + l * 64) * REGF; J.nrep = 1;
                    if (l == 0) { J.B = stash + (size_t)PDE_X0 * REGF; J.b_regs = 16; J.bmode = BM_RAW; }
                    else { J.B = stash + (size_t)(z + (l - 1) * 64) * REGF; J.b_regs = 64; J.bmode = net == 1 ? BM_RELU : BM_SILU; }
                } else {                      // 4 tangent columns of weight_net (no bias term)
                    J.A = stash + (size_t)(PDE_GA + 336 + l * 64) * REGF; J.nrep = 4; J.a_rep_stride = (size_t)336 * REGF;
                    if (l == 0) { J.B = stash + (size_t)PDE_X0D * REGF; J.b_regs = 16; J.bmode = BM_RAW; J.b_rep_stride = (size_t)16 * REGF; }
                    else {
                        J.B = stash + (size_t)(PDE_Z + (l - 1) * 64) * REGF; J.b_rep_stride = 0;
                        J.B2 = stash + (size_t)(PDE_ZD + (l - 1) * 64) * REGF; J.b2_rep_stride = (size_t)320 * REGF;
                        J.b_regs = 64; J.bmode = BM_SILU_TAN;
                    }
                }
            }
            const int a_regs = l < 5 ? 64 : 16, b_regs = l == 0 ? 16 : 64;
            // weights: value (+ tangent) slabs; bias: value slabs only (tangent columns carry no bias term)
            ReduceJob& Q = rj.j[rj.n++];
            memset(&Q, 0, sizeof(Q));
            Q.slabs = sl[0]; Q.nslab = PDE_NSLAB; Q.slabs2 = sl[1]; Q.nslab2 = sl[1] ? PDE_NSLAB : 0;
            Q.MTA = a_regs / 16; Q.KTB = b_regs / 16; Q.gW = gW; Q.gb = nullptr;
            Q.out = l < 5 ? 128 : 6; Q.in = l == 0 ? 28 : 128; Q.row_kind = RK_NATURAL; Q.slot_kind = l == 0 ? SK_VEL_IN : SK_HIDDEN; Q.scale = 1.f;
            if (gb) {
                ReduceJob& Qb = rj.j[rj.n++];
                Qb = Q; Qb.slabs2 = nullptr; Qb.nslab2 = 0; Qb.gW = nullptr; Qb.gb = gb;
            }
        }
    if (launch_wgrad(wj, rj, st)) return 1;
    return 0;
}
