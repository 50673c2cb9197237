// abi.hip - error plumbing, version, self test and the small building-block entry points of the C ABI.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "pde.h"
#include "render.h"
#include "x6.h"
#include "warp.h"

static thread_local char g_err[512] = "";
int nvfi_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* nvfi_last_error(void) { return g_err; }

// ---------------------------------------------------------------- environment switches (switches.h)
static int parse_INT(Switch, const char* text) { return atoi(text); }
static int parse_WORD(Switch s, const char* text) {
    if (s == NVFI_SCATTER) return !strcmp(text, "lds") ? SCATTER_LDS : SCATTER_MFMA;
    static const struct { const char* word; int value; } pre[] = {{"fp32", PRE_FP32}, {"split32", PRE_FP32}, {"x6", PRE_X6}, {"fp16band", PRE_FP16BAND}, {"split16band", PRE_SPLIT16BAND}};
    for (const auto& p : pre) if (!strcmp(text, p.word)) return p.value;
    return PRE_UNKNOWN;
}
int sw(Switch s) {
    static std::once_flag once;
    static int value[NVFI_SWITCH_COUNT];
    std::call_once(once, [] {
#define X(name, kind, def) { const char* e = getenv(#name); value[name] = parse_##kind(name, e ? e : #def); }
        NVFI_SWITCHES(X)
#undef X
    });
    return value[s];
}
extern "C" int nvfi_abi_version(void) { return NVFI_ABI_VERSION; }
extern "C" int nvfi_stream_capture_id(void* stream, uint64_t* id) {
    hipStreamCaptureStatus stt = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    HIPCK(hipStreamGetCaptureInfo((hipStream_t)stream, &stt, &cid));
    *id = stt == hipStreamCaptureStatusActive ? (uint64_t)cid + 1 : 0;
    return 0;
}

// ---------------------------------------------------------------- VelBasis evaluation
// ONE published size for the workspaces of nvfi_vel_eval (both nets' fragments) and nvfi_integrate_pos (PosPlan below); nvfi_char_loss nests it
static_assert(VEL_FRAG_FLOATS * 4 % 256 == 0 && VEL_FRAG_FLOATS * 4 + 4096 >= X6_IMAGE_BYTES + 256,
              "nvfi_vel_workspace_bytes covers PosPlan: one fragment set, N float4 (up to 240 bytes of padding behind them) and the x6 image");
extern "C" int nvfi_vel_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes) {
    (void)f;
    *bytes = align_up((int64_t)2 * VEL_FRAG_FLOATS * 4 + 4096 + N * 16 + N * 12, 256);
    return 0;
}
extern "C" int nvfi_vel_eval(const nvfi_field_desc* f, int64_t N, const float* xt, float* u6, int gated,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (check_vel_call("nvfi_vel_eval", f, 0, VEL_CALL_DESC)) return 2;      // (N is bounded by the workspace alone)
    if (N <= 0) return 0;
    // the published size (nvfi_vel_workspace_bytes) is the contract, as in nvfi_compute_alpha: anything under it is refused here
    int64_t need = 0; nvfi_vel_workspace_bytes(f, N, &need);
    if (need > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)need);
    Bump B{(char*)workspace, 0, 0};
    float* fv = B.take<float>(VEL_FRAG_FLOATS);
    float* fa = B.take<float>(VEL_FRAG_FLOATS);
    VelImages VI;
    if (int rc = vel_images(f, gated ? VI_VEL : VI_VEL | VI_ANET, VelImageRoom{fv, fa}, &VI, nullptr, 0, st)) return rc;
    VelEvalArgs a; memset(&a, 0, sizeof(a));
    a.f = *f; a.Wv = VI.VW; a.Wa = VI.AW; a.N = N; a.xt = xt; a.u6 = u6; a.gated = gated;
    return launch_vel_eval(a, st);
}

// ---------------------------------------------------------------- integrate_pos (per-point times)
__global__ void k_pack_xt(int64_t N, const float* x, float4* xw) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < N) xw[i] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], 0.f);
}
// fv: the fp32 fragments (WARP_FP32) or the fp16 images, hi + lo (WARP_FP16IN: the fragment region is that warp's img16); x6img: the call's
// own x6 image (WARP_X6 without a fragment cache)
struct PosPlan { float* fv; float4* xw; float* x6img; int64_t total; };
static_assert(VEL_FRAG_FLOATS * 4 >= 2 * PRE16_IMAGE_BYTES, "fragment region holds the fp16 images (hi + lo)");
static void plan_pos(const nvfi_field_desc* f, WarpKind kind, int64_t N, void* ws, PosPlan* P) {
    Bump B{(char*)ws, 0, 0};
    const unsigned own = f->frags ? 0 : warp_need(kind, WARP_POINTS);
    P->fv = B.take<float>(VEL_FRAG_FLOATS);
    P->xw = B.take<float4>(N);
    P->x6img = (own & VI_X6) ? B.take<float>(X6_IMAGE_BYTES / 4) : nullptr;
    P->total = B.off;
}
extern "C" int nvfi_integrate_pos(const nvfi_field_desc* f, int64_t N, const float* x, const float* t, const float* base,
                                  float* xk, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (check_vel_call("nvfi_integrate_pos", f, N, VEL_CALL_DESC)) return 2;       // (in front of the empty call's 0)
    if (N <= 0) return 0;
    int64_t need = 0; nvfi_vel_workspace_bytes(f, N, &need);      // the published size covers every PosPlan (static_assert above)
    if (need > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)need);
    const WarpKind kind = warp_kind(f, false, true);
    PosPlan P; plan_pos(f, kind, N, workspace, &P);
    VelImages VI;
    if (int rc = vel_images(f, warp_need(kind, WARP_POINTS), VelImageRoom{P.fv, nullptr, nullptr, nullptr, nullptr, P.x6img}, &VI, nullptr, 0, st)) return rc;
    hipLaunchKernelGGL(k_pack_xt, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, x, P.xw);
    return warp_points(f, kind, VI, P.fv, WarpPoints{nullptr, N, nullptr, P.xw, xk, t, base, 0, 4096}, st);
}

// ---------------------------------------------------------------- compute_alpha / device-side rays (next rows f-3, f-2)
__global__ void k_alpha_prep(nvfi_field_desc f, int64_t N, const float* xyz, float tn, float4* xw) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < N) xw[i] = make_float4(norm_coord(f, 0, xyz[3 * i]), norm_coord(f, 1, xyz[3 * i + 1]), norm_coord(f, 2, xyz[3 * i + 2]), tn);
}
__global__ void k_alpha_finish(int64_t N, const float* sig, float length, int acc_max, float* out) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float a = 1.f - expf(-sig[i] * length);
    out[i] = acc_max ? fmaxf(out[i], a) : a;
}
struct AlphaPlan { float* fv; float4* xw; float* sig; float* x6img; int64_t total; };
static void plan_alpha(int64_t N, void* ws, AlphaPlan* P) {
    Bump B{(char*)ws, 0, 0};
    P->fv = B.take<float>(VEL_FRAG_FLOATS);
    P->xw = B.take<float4>(N);
    P->sig = B.take<float>(N);
    P->x6img = B.take<float>(X6_IMAGE_BYTES / 4);
    P->total = align_up(B.off, 256);
}
// the per-point times of the x6 kernel for a call whose time is uniform (X6Args has no stride-0 form: the two values are broadcast into
// N-element arrays behind the plan)
__global__ void k_alpha_times(int64_t N, float t, float base, float* tt, float* tb) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < N) { tt[i] = t; tb[i] = base; }
}
extern "C" int nvfi_alpha_workspace_bytes(const nvfi_field_desc* f, int64_t N, int64_t* bytes) {
    (void)f;
    AlphaPlan P; plan_alpha(N > 0 ? N : 0, nullptr, &P);
    *bytes = P.total + align_up(2 * (N > 0 ? N : 0) * (int64_t)sizeof(float), 256);
    return 0;
}
extern "C" int nvfi_compute_alpha(const nvfi_field_desc* f, int64_t N, const float* xyz_world, float t, int transfer, float length,
                                  int accumulate_max, float* alpha_out, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (N <= 0) return 0;
    if (N >= POINTS_PER_CALL_MAX) return nvfi_fail(2, "N too large for one call; chunk the points");
    AlphaPlan AP; plan_alpha(N, workspace, &AP);
    float* fv = AP.fv; float4* xw = AP.xw; float* sig = AP.sig;
    // the published size (nvfi_alpha_workspace_bytes) is the contract whichever integrator the call takes: refused here, before anything is launched
    const int64_t need = AP.total + align_up(2 * N * (int64_t)sizeof(float), 256);
    if (need > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)need);
    // the uniform step sequence back to the keyframe (0: t IS the keyframe time or the field has no velocity net).  Not the render's rk_schedule:
    // the reference's compute_alpha has no isclose shortcut - integrate_pos steps while t - base != 0, however small (tensorf_keyframe.py:508-537)
    Rk2Args a; memset(&a, 0, sizeof(a));
    const float base = transfer ? 0.f : snap_base(*f, t);
    const int n = f->use_vel ? rk_steps(dt_max_of(*f), t, base, a.dt, a.tcur) : 0;
    const WarpKind kind = warp_kind(f, false, true);
    const unsigned nb = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(k_alpha_prep, dim3(nb), dim3(256), 0, st, *f, N, xyz_world, norm_time(*f, base), xw);
    VelImages VI;
    if (n != 0 && kind == WARP_X6) {
        // round 6: the x6 kernel with per-point times (all equal here; the kernel runs integrate_pos' own fp32 recurrence dt = sign * min(|off|,
        // dt_max) per point: the schedule's numbers, without its limit of MAX_RK_STEPS).  tt / tb: 2 N floats behind the plan (nvfi_alpha_workspace_bytes)
        float* tt = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + AP.total);
        float* tb = tt + N;
        if (AP.total + 2 * N * (int64_t)sizeof(float) > workspace_bytes) return nvfi_fail(4, "workspace too small: need %lld", (long long)(AP.total + 8 * N));
        if (int rc = vel_images(f, warp_need(kind, WARP_POINTS), VelImageRoom{nullptr, nullptr, nullptr, nullptr, nullptr, AP.x6img}, &VI, nullptr, 0, st)) return rc;
        hipLaunchKernelGGL(k_alpha_times, dim3(nb), dim3(256), 0, st, N, t, base, tt, tb);
        if (warp_points(f, kind, VI, nullptr, WarpPoints{nullptr, N, nullptr, xw, nullptr, tt, tb, 0, 4096}, st)) return 1;
    } else if (n != 0) {
        if (n < 0) return nvfi_fail(2, "t=%g needs more than %d RK2 steps", t, MAX_RK_STEPS);
        if (kind == WARP_FP16IN) {  // opt-in fp16-input inference mode (pre16.hip)
            Rk16Args h; memset(&h, 0, sizeof(h));
            h.img = fv; h.P = N; h.xw = xw; h.xout = xw; h.nsteps = n;
            for (int k = 0; k < n; ++k) { h.dt[k] = a.dt[k]; h.tcur[k] = a.tcur[k]; }
            if (launch_rk2_inf16(f, h, true, st)) return 1;
        } else {
            if (int rc = vel_images(f, VI_VEL, VelImageRoom{fv}, &VI, nullptr, 0, st)) return rc;
            a.f = *f; a.Wv = VI.VW; a.count = nullptr; a.n_direct = N; a.list = nullptr; a.xw = xw; a.xout = nullptr; a.nsteps = n;
            if (launch_rk2_fwd(a, N, true, st)) return 1;
        }
    }
    {   // density at the (warped) points with the quad-lane gather kernel (scatter.hip), then alpha = 1 - exp(-sigma * length)
        DensityArgs da; memset(&da, 0, sizeof(da));
        da.f = *f; da.n_direct = N; da.xw = xw; da.per_point_t = 1; da.sigma_out = sig;
        if (launch_density_q(da, N, st)) return 1;
    }
    hipLaunchKernelGGL(k_alpha_finish, dim3(nb), dim3(256), 0, st, N, sig, length, accumulate_max, alpha_out);
    LAUNCHCK();
    return 0;
}

__global__ void k_gen_rays(const float* __restrict__ pose, int H, int W, float focal, int64_t n, const int64_t* __restrict__ ids,
                           float* __restrict__ ro, float* __restrict__ rd) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t pid = ids ? ids[i] : i;
    const float X = (float)(pid % W), Y = (float)(pid / W);
    // directions = ((X - W/2)/focal, -(Y - H/2)/focal, -1); ray_d = sum(directions * pose[:3,:3], -1) (camera.py:112-131)
    const float d0 = (X - W * 0.5f) / focal, d1 = -(Y - H * 0.5f) / focal, d2 = -1.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rd[3 * i + r] = d0 * pose[4 * r + 0] + d1 * pose[4 * r + 1] + d2 * pose[4 * r + 2];
        ro[3 * i + r] = pose[4 * r + 3];
    }
}
extern "C" int nvfi_gen_rays(const float* pose3x4, int H, int W, float focal, int64_t n, const int64_t* pixel_ids, float* rays_o, float* rays_d, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_gen_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pose3x4, H, W, focal, n, pixel_ids, rays_o, rays_d);
    LAUNCHCK();
    return 0;
}

// ---------------------------------------------------------------- the random inputs of one training iteration in one launch (round 5)
// What the reference draws per iteration (train_nvfi.py:150-178: a pixel batch per render via Camera.sample_rays; models/nvfi.py:44-47: the
// collocation points `torch.rand(n,3) * (max - min) + min` and times `torch.rand(n,1)` of get_vel_loss) took ~13 torch launches in the fused
// driver (randint, two index gathers and a rand per render; two rands, a subtract, a multiply and an add for the points).  Here one kernel
// fills all of it from a counter-based generator: Philox4x32-10 (Salmon et al., SC'11) keyed by `seed`, counter = (element, segment,
// iteration) - thread i produces the four words of ray i of a batch (pixel index + three target channels) or of point i (x, y, z, t).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.f / 16777216.f); }     // [0, 1): 24 random bits, like torch.rand
// a bijection of [0, n): four-round balanced Feistel network on the smallest 4^half >= n, cycle-walked back into range (x < n stays on
// its own cycle, so distinct inputs give distinct outputs): pixel r of a batch is perm(r) - R DISTINCT pixels, as Camera.sample_rays'
// np.random.choice(..., replace=False) draws them (models/camera.py:160)
__device__ __forceinline__ unsigned feistel_perm(unsigned r, unsigned n, const unsigned (&key)[4]) {
    if (n <= 1) return 0;
    const int bits = 32 - __clz((int)(n - 1));
    const int half = (bits + 1) >> 1;
    const unsigned mask = (1u << half) - 1u;
    unsigned x = r;
    do {
        unsigned L = x >> half, R = x & mask;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned f = (R + key[k]) * 0x9E3779B1u;
            f ^= f >> 15; f *= 0x85EBCA77u; f ^= f >> 13;
            const unsigned nl = R;
            R = (L ^ f) & mask; L = nl;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}
__global__ __launch_bounds__(256) void k_draw_batch(nvfi_draw_desc a) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const unsigned long long it = a.iteration_dev ? *a.iteration_dev : a.iteration;
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    unsigned w[4];
    if (i < a.R * a.n_batches) {
        const int b = (int)(i / a.R);
        const int64_t r = i - (int64_t)b * a.R;
        unsigned key[4];
        philox4x32_10(0xffffffffu, 0x40000000u | (unsigned)b, (unsigned)it, (unsigned)(it >> 32), k0, k1, key);     // the batch's permutation key
        philox4x32_10((unsigned)r, (unsigned)b, (unsigned)it, (unsigned)(it >> 32), k0, k1, w);
        const int64_t pix = (int64_t)feistel_perm((unsigned)r, (unsigned)a.n_pixels, key);     // R distinct pixels of [0, n_pixels)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.rays_o[b][3 * r + c] = a.bundle_o[3 * pix + c];
            a.rays_d[b][3 * r + c] = a.bundle_d[3 * pix + c];
            a.target[b][3 * r + c] = a.target_img ? a.target_img[3 * pix + c] : u01(w[1 + c]);
        }
        if (a.pixel_ids[b]) a.pixel_ids[b][r] = pix;
    }
    if (i < a.P) {
        philox4x32_10((unsigned)i, 0x80000000u | (unsigned)(i >> 32), (unsigned)it, (unsigned)(it >> 32), k0, k1, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.points[3 * i + c] = u01(w[c]) * (a.aabb[3 + c] - a.aabb[c]) + a.aabb[c];      // models/nvfi.py:45
        a.t[i] = u01(w[3]);
    }
}
extern "C" int nvfi_draw_batch(const nvfi_draw_desc* d, void* stream) {
    if (d->n_batches < 0 || d->n_batches > 2) return nvfi_fail(2, "nvfi_draw_batch: n_batches must be 0, 1 or 2");
    if (d->n_batches > 0 && (d->R <= 0 || d->n_pixels <= 0 || !d->bundle_o || !d->bundle_d)) return nvfi_fail(2, "nvfi_draw_batch: ray batches need R, n_pixels and the camera bundle");
    if (d->n_batches > 0 && (d->R > d->n_pixels || d->n_pixels >= (1ll << 31)))
        return nvfi_fail(2, "nvfi_draw_batch: R = %lld distinct pixels of %lld (the draw is without replacement, like np.random.choice(replace=False))", (long long)d->R, (long long)d->n_pixels);
    for (int b = 0; b < d->n_batches; ++b) if (!d->rays_o[b] || !d->rays_d[b] || !d->target[b]) return nvfi_fail(2, "nvfi_draw_batch: batch %d has a NULL output", b);
    if (d->P > 0 && (!d->points || !d->t)) return nvfi_fail(2, "nvfi_draw_batch: points / t are NULL");
    int64_t n = d->R * d->n_batches;
    if (d->P > n) n = d->P;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_draw_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d);
    LAUNCHCK();
    return 0;
}

// ---------------------------------------------------------------- MFMA layout self test
__global__ __launch_bounds__(WG_THREADS) void k_selftest(const float* frag, const float* W, const float* X, float* out) {
    // one workgroup, wave 0 only does the maths: out[o][j] = sum_k W[o][k] X[k][j], 128x128 by 128x32
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    stage_frag(lds, lds + LDS_W_FLOATS, frag, 4 * 64 * 64, nullptr, 0);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    float x[64];
#pragma unroll
    for (int s = 0; s < 64; ++s) x[s] = X[dmap(s, h) * 32 + j];
    f32x16 acc[4];
    acc_init<4>(acc, lds, 0, false);
    layer_mfma<4, 64>(lds, lane, x, acc);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[dmap(16 * m + r, h) * 32 + j] = acc[m][r];
}
extern "C" int nvfi_selftest(float* max_err_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int O = 128, K = 128, J = 32;
    float *hW = new float[O * K], *hX = new float[K * J], *hO = new float[O * J];
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.f - 0.5f; };
    for (int i = 0; i < O * K; ++i) hW[i] = rnd();
    for (int i = 0; i < K * J; ++i) hX[i] = rnd();
    float *dW, *dX, *dO, *dF;
    HIPCK(hipMalloc(&dW, O * K * 4)); HIPCK(hipMalloc(&dX, K * J * 4)); HIPCK(hipMalloc(&dO, O * J * 4)); HIPCK(hipMalloc(&dF, 4 * 64 * 64 * 4));
    HIPCK(hipMemcpyAsync(dW, hW, O * K * 4, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dX, hX, K * J * 4, hipMemcpyHostToDevice, st));
    PackJobs jobs; jobs.n = 1;
    PackJob& P = jobs.j[0];
    P.W = dW; P.b = nullptr; P.frag = dF; P.bfrag = nullptr; P.out = O; P.in = K; P.MT = 4; P.NS = 64;
    P.row_kind = RK_NATURAL; P.slot_kind = SK_HIDDEN; P.transposed = 0; P.x4 = 0;
    if (launch_pack(jobs, st)) return 1;
    static DeviceOnce once;
    if (once.lds(ENGINE_LDS_BYTES, k_selftest)) return 1;
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, dF, dW, dX, dO);
    LAUNCHCK();
    HIPCK(hipMemcpyAsync(hO, dO, O * J * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    float me = 0.f;
    for (int o = 0; o < O; ++o)
        for (int j = 0; j < J; ++j) {
            float r = 0.f;
            for (int k = 0; k < K; ++k) r += hW[o * K + k] * hX[k * J + j];
            float e = fabsf(r - hO[o * J + j]);
            if (e > me) me = e;
        }
    *max_err_host = me;
    (void)hipFree(dW); (void)hipFree(dX); (void)hipFree(dO); (void)hipFree(dF);
    delete[] hW; delete[] hX; delete[] hO;
    return 0;
}

// ---------------------------------------------------------------- activation / encoding primitives, exposed for the ULP tests
__global__ void k_debug_act(int kind, int64_t n, const float* __restrict__ x, float* __restrict__ y) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    float r = 0.f, d1, d2;
    switch (kind) {
        case 0: r = fast_sigmoid(v); break;
        case 1: r = trig_sel(v, 0); break;
        case 2: r = trig_sel(v, 1); break;
        case 3: r = act_f<1>(v); break;
        case 4: r = act_d1<1>(v); break;
        case 5: act_d12<1>(v, d1, d2); r = d2; break;
        default: break;
    }
    y[i] = r;
}
extern "C" int nvfi_debug_act(int kind, int64_t n, const float* x, float* y, void* stream) {
    if (n <= 0) return 0;
    if (kind < 0 || kind > 5) return nvfi_fail(2, "nvfi_debug_act: kind %d outside 0..5", kind);
    hipLaunchKernelGGL(k_debug_act, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kind, n, x, y);
    LAUNCHCK();
    return 0;
}

// ---------------------------------------------------------------- PDE entry points live in pde.hip

// ---------------------------------------------------------------- per-kernel-class event timing
#include <vector>
static int g_prof = 0;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_ev[PK_COUNT];
static std::vector<hipEvent_t> g_pool;
static hipEvent_t g_open[PK_COUNT];
static hipEvent_t ev_get() {
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void prof_begin(int cls, hipStream_t st) {
    if (!g_prof) return;
    g_open[cls] = ev_get();
    (void)hipEventRecord(g_open[cls], st);
}
void prof_end(int cls, hipStream_t st) {
    if (!g_prof) return;
    hipEvent_t e = ev_get();
    (void)hipEventRecord(e, st);
    g_ev[cls].push_back({g_open[cls], e});
}
// marks the start of a profiled pass in a rocprofv3 kernel trace (tools/rocpd_stats.py summarises the launches after the last marker)
__global__ void k_nvfi_prof_marker(int on) { (void)on; }
extern "C" int nvfi_prof_enable(int on) {
    if (on) { hipLaunchKernelGGL(k_nvfi_prof_marker, dim3(1), dim3(64), 0, 0, on); (void)hipStreamSynchronize(0); }
    g_prof = on;
    for (int c = 0; c < PK_COUNT; ++c) { for (auto& p : g_ev[c]) { g_pool.push_back(p.first); g_pool.push_back(p.second); } g_ev[c].clear(); }
    return 0;
}
/* total_ms[PK_COUNT], count[PK_COUNT] (host arrays); synchronises the recorded events */
extern "C" int nvfi_prof_collect(double* total_ms, int64_t* count) {
    for (int c = 0; c < PK_COUNT; ++c) {
        double t = 0.0;
        for (auto& p : g_ev[c]) {
            HIPCK(hipEventSynchronize(p.second));
            float ms = 0.f;
            HIPCK(hipEventElapsedTime(&ms, p.first, p.second));
            t += ms;
        }
        total_ms[c] = t; count[c] = (int64_t)g_ev[c].size();
    }
    return 0;
}
extern "C" int nvfi_prof_nclasses(void) { return PK_COUNT; }
