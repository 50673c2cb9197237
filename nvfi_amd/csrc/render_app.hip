// render_app.hip - the appearance branch of the render on the fp32 MFMA engine: plane-product features -> basis_mat -> positional encodings
// -> MLPRender_PE (or the SH epilogue) per masked sample, and its adjoint down to the per-sample channel gradients of the planes.
// Reference semantics: models/tensorf_base.py:67-98 (MLPRender_PE), models/tensorf_model_utils.py:176-183 (PE), 292-296 (SHRender).
#include "common.h"
#include "render.h"

// ================================================================ appearance (MFMA)
// Per-lane scratch in the (idle) weight LDS region: row k of thread tid lives at scr[k*256 + tid].
// Loop-computed values (gathers, sincos) go through it so that the big register arrays keep static indices.
#define SCR_OFF (8 * 256)

__device__ __forceinline__ void app_gather_to_scratch(const nvfi_field_desc& f, const Bl* b, int h, float* scr) {
    // lane (j,h) holds channels 4*(2a+h)+c, a=0..5  (= the B-operand layout of the basis_mat layer)
#pragma unroll 1
    for (int a6 = 0; a6 < 6; ++a6) {
        const int q4 = 2 * a6 + h;
        float4 s0 = bl_sample4(f.aps[0], f.Ca, b[0], q4), s1 = bl_sample4(f.aps[1], f.Ca, b[1], q4), s2 = bl_sample4(f.aps[2], f.Ca, b[2], q4);
        float4 t0 = bl_sample4(f.apt[0], f.Ca, b[3], q4), t1 = bl_sample4(f.apt[1], f.Ca, b[4], q4), t2 = bl_sample4(f.apt[2], f.Ca, b[5], q4);
        scr[(4 * a6 + 0) * 256 + threadIdx.x] = ((s0.x * s1.x) * s2.x) * ((t0.x * t1.x) * t2.x);
        scr[(4 * a6 + 1) * 256 + threadIdx.x] = ((s0.y * s1.y) * s2.y) * ((t0.y * t1.y) * t2.y);
        scr[(4 * a6 + 2) * 256 + threadIdx.x] = ((s0.z * s1.z) * s2.z) * ((t0.z * t1.z) * t2.z);
        scr[(4 * a6 + 3) * 256 + threadIdx.x] = ((s0.w * s1.w) * s2.w) * ((t0.w * t1.w) * t2.w);
    }
}

template <bool STASH>
__global__ __launch_bounds__(WG_THREADS, 2) void k_app_fwd(AppArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int count = a.count ? *a.count : (int)a.n_direct;
    if ((int)(blockIdx.x * WG_SAMPLES) >= count) return;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = i < count;
    const int n = active ? (a.list ? a.list[i] : i) : 0;
    float4 q = active ? a.xw[n] : zero4();
    const float tn = a.per_point_t ? q.w : SCHED_TN(a);
    float vd[3] = {0.f, 0.f, 0.f};
    if (active) {
        const float* vp = a.view_per_point ? a.view_per_point + 3 * (size_t)n : a.rays_d + 3 * (size_t)(n / a.S);
        vd[0] = vp[0]; vd[1] = vp[1]; vd[2] = vp[2];
    }
    float x[64];
    float* scr = lds_w + SCR_OFF;
    if (a.feat48) {
        // lane (j,h) holds channels 4*(2a+h)+c, a=0..5, of its sample
        const float* fp = a.feat48 + (size_t)(active ? i : 0) * 48 + 4 * h;
#pragma unroll
        for (int a6 = 0; a6 < 6; ++a6) {
            const float4 v = active ? ld4(fp + 8 * a6) : zero4();
            x[4 * a6 + 0] = v.x; x[4 * a6 + 1] = v.y; x[4 * a6 + 2] = v.z; x[4 * a6 + 3] = v.w;
        }
    } else {
        if (!a.feat_in) {
            Bl b[6];
            plane_setups(f, q.x, q.y, q.z, tn, b);
            app_gather_to_scratch(f, b, h, scr);
        }
#pragma unroll
        for (int s = 0; s < 24; ++s) x[s] = a.feat_in ? 0.f : scr[s * 256 + threadIdx.x];
    }
    float* st = STASH ? a.stash_f + (size_t)tile * (APP_F_ROWS * REGF) : nullptr;
    if (STASH) {
#pragma unroll
        for (int s = 0; s < 32; ++s) STASH_ST(st[s * REGF + lane], s < 24 ? x[s] : 0.f);
    }
    // positional encodings (tensorf_model_utils.py:176-183) -> scratch rows 0..35 (sin|cos selected by h)
#pragma unroll 1
    for (int e = 0; e < 18; ++e) {
        const int c = e / 6, k = e - 6 * c;
        const float fr = (float)(1 << k);
        const float pc = c == 0 ? q.x : (c == 1 ? q.y : q.z);
        const float vc = c == 0 ? vd[0] : (c == 1 ? vd[1] : vd[2]);
        scr[e * 256 + threadIdx.x] = trig_sel(pc * fr, h);
        scr[(18 + e) * 256 + threadIdx.x] = trig_sel(vc * fr, h);
    }
    // basis_mat: 48 -> 32 (no bias); its fragment occupies LDS rows below SCR_OFF
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.fb, RF_B, nullptr, 0);
    __syncthreads();
    f32x16 o1[1];
    acc_init<1>(o1, lds_b, h, false);
    if (!a.feat_in) layer_mfma<1, 24>(lds_w, lane, x, o1);
    else {      // features from the caller, in the D layout of the basis tile: register r of lane (n, h) is feature (r&3) + 8(r>>2) + 4h
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            o1[0][r] = (active && row < f.app_dim) ? a.feat_in[(size_t)n * f.app_dim + row] : 0.f;
        }
    }
    if (f.shading == 1) {
        // SHRender (tensorf_model_utils.py:292-296, sh.py:87-110): the 27 features are rows (r&3)+8(r>>2)+4h of the basis tile, split over the
        // lane pair (l, l+32); colour c = relu(sum_k SH_k(viewdir) feat[9c + k] + 0.5).  No MLP, no positional encodings.
        float sh[9];
        sh_bases9(vd, sh);
        float part[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < 27) part[row / 9] += sh[row % 9] * o1[0][r];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) part[c] += __shfl_xor(part[c], 32);
        if (active && h == 0) {
            float4 c = make_float4(fmaxf(part[0] + 0.5f, 0.f), fmaxf(part[1] + 0.5f, 0.f), fmaxf(part[2] + 0.5f, 0.f), 0.f);
            a.rgbs[a.rgb_dense ? n : i] = c;
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = o1[0][r];
    x[16] = h ? q.x : vd[0]; x[17] = h ? q.y : vd[1]; x[18] = h ? q.z : vd[2];
#pragma unroll
    for (int e = 0; e < 18; ++e) { x[19 + e] = scr[e * 256 + threadIdx.x]; x[37 + e] = scr[(18 + e) * 256 + threadIdx.x]; }
#pragma unroll
    for (int s = 55; s < 64; ++s) x[s] = 0.f;
    if (STASH) stash_store<64>(st + 32 * REGF, lane, x);
    f32x16 acc[4];
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f1, RF_1, a.W.b1, 128);
    __syncthreads();
    acc_init<4>(acc, lds_b, h, true);
    layer_mfma<4, 55>(lds_w, lane, x, acc);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[16 * m + r] = fmaxf(acc[m][r], 0.f);
    if (STASH) stash_store<64>(st + 96 * REGF, lane, x);
    if (STASH) relu_mask_store(a.relu_mask + (size_t)tile * 256, lane, x);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f2, RF_2, a.W.b2, 128);
    __syncthreads();
    acc_init<4>(acc, lds_b, h, true);
    layer_mfma<4, 64>(lds_w, lane, x, acc);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[16 * m + r] = fmaxf(acc[m][r], 0.f);
    if (STASH) stash_store<64>(st + 160 * REGF, lane, x);
    if (STASH) relu_mask_store(a.relu_mask + (size_t)tile * 256 + 128, lane, x);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.f3, RF_3, a.W.b3, 32);
    __syncthreads();
    acc_init<1>(o1, lds_b, h, true);
    layer_mfma<1, 64>(lds_w, lane, x, o1);
    if (active && h == 0) {
        float4 c = make_float4(sigmoid_f(o1[0][0]), sigmoid_f(o1[0][1]), sigmoid_f(o1[0][2]), 0.f);
        a.rgbs[a.rgb_dense ? n : i] = c;
    }
}

// backward of the appearance branch for masked samples
__global__ __launch_bounds__(WG_THREADS, 2) void k_app_bwd(AppArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* lds_w = lds; float* lds_b = lds + LDS_W_FLOATS;
    const nvfi_field_desc& f = a.f;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int count = *a.count;
    if ((int)(blockIdx.x * WG_SAMPLES) >= count) return;
    const int tile = blockIdx.x * 4 + wave_id();
    const int i = tile * TILE + (lane & 31);
    const bool active = i < count;
    const int n = active ? a.list[i] : 0;
    const float* stf = a.stash_f + (size_t)tile * (APP_F_ROWS * REGF);
    float* stb = a.stash_b + (size_t)tile * (APP_B_ROWS * REGF);
    float g[64];
    f32x16 acc[4];
    float gpts[3];
    if (f.shading == 1) {
        // SHRender backward: d pre_c = w * gr_c where the stored colour is positive (relu'), d feat[9c + k] = SH_k(viewdir) * d pre_c
        float gpre[3] = {0.f, 0.f, 0.f};
        float vd[3] = {0.f, 0.f, 0.f};
        if (active) {
            const int r = n / a.S;
            const float* vp = a.rays_d + 3 * (size_t)r;
            vd[0] = vp[0]; vd[1] = vp[1]; vd[2] = vp[2];
            if (a.g_rgb) {
                const float4 pre = a.rgb_pre[r];
                const float pv[3] = {pre.x, pre.y, pre.z};
                const float4 c = a.rgbs[i];
                const float cv[3] = {c.x, c.y, c.z};
                const float w = a.weight[n];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float gr = (pv[k] >= 0.f && pv[k] <= 1.f) ? a.g_rgb[3 * (size_t)r + k] : 0.f;
                    gpre[k] = cv[k] > 0.f ? w * gr : 0.f;
                }
            }
        }
        float sh[9];
        sh_bases9(vd, sh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            acc[0][r] = row < 27 ? sh[row % 9] * gpre[row / 9] : 0.f;
        }
        gpts[0] = gpts[1] = gpts[2] = 0.f;
    } else {
    // seeds: go_c = w * gr_c * c(1-c) in rows 0..2 of a D tile (lane h=0 regs 0..2)
    {
        float go[3] = {0.f, 0.f, 0.f};
        if (active && h == 0 && a.g_rgb) {
            const int r = n / a.S;
            const float4 pre = a.rgb_pre[r];
            const float pv[3] = {pre.x, pre.y, pre.z};
            const float4 c = a.rgbs[i];
            const float cv[3] = {c.x, c.y, c.z};
            const float w = a.weight[n];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float gr = (pv[k] >= 0.f && pv[k] <= 1.f) ? a.g_rgb[3 * (size_t)r + k] : 0.f;
                go[k] = w * gr * cv[k] * (1.f - cv[k]);
            }
        }
        g[0] = go[0]; g[1] = go[1]; g[2] = go[2]; g[3] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) STASH_ST(stb[s * REGF + lane], s < 3 ? g[s] : 0.f);
    }
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t3, RT_3, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 4>(lds_w, lane, g, acc);
    {
        const unsigned* mk = a.relu_mask + (size_t)tile * 256 + 128;
        const unsigned mlo = mk[lane], mhi = mk[64 + lane];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[16 * m + r] = (((m < 2 ? mlo : mhi) >> ((16 * m + r) & 31)) & 1u) ? acc[m][r] : 0.f;
    }
    stash_store<64>(stb + 16 * REGF, lane, g);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t2, RT_2, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 64>(lds_w, lane, g, acc);
    {
        const unsigned* mk = a.relu_mask + (size_t)tile * 256;
        const unsigned mlo = mk[lane], mhi = mk[64 + lane];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[16 * m + r] = (((m < 2 ? mlo : mhi) >> ((16 * m + r) & 31)) & 1u) ? acc[m][r] : 0.f;
    }
    stash_store<64>(stb + 80 * REGF, lane, g);
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.t1, RT_1, nullptr, 0);
    __syncthreads();
    acc_init<4>(acc, lds_b, 0, false);
    layer_mfma<4, 64>(lds_w, lane, g, acc);
    // acc = gradient wrt the 110 input slots (RENDER_IN layout)
    {
        const float* xin = stf + 32 * REGF;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = h ? acc[1][c] : 0.f;          // slots 16..18: h=1 holds raw pts
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int sl = 19 + c * 6 + k;
                const float mine = STASH_LD(xin[sl * REGF + lane]);
                const float other = __shfl_xor(mine, 32);
                const float fr = (float)(1 << k);
                s += (h ? -fr * other : fr * other) * acc[sl >> 4][sl & 15];
            }
            s += __shfl_xor(s, 32);
            gpts[c] = s;
        }
    }
    }   // MLP_PE
    // gfeat (tile 0) -> stash, then basis^T -> gg (48 channels in gather layout)
#pragma unroll
    for (int r = 0; r < 16; ++r) { g[r] = acc[0][r]; STASH_ST(stb[(144 + r) * REGF + lane], g[r]); }
    __syncthreads();
    stage_frag(lds_w, lds_b, a.W.tb, RT_B, nullptr, 0);
    __syncthreads();
    f32x16 gg[2];
    acc_init<2>(gg, lds_b, 0, false);
    layer_mfma<2, 16>(lds_w, lane, g, gg);
    // plane backward for this lane's 24 channels (channel grads via LDS scratch -> non-unrolled loop)
    float* scr = lds_w + SCR_OFF;
    __syncthreads();
#pragma unroll
    for (int s2 = 0; s2 < 24; ++s2) scr[s2 * 256 + threadIdx.x] = active ? gg[s2 >> 4][s2 & 15] : 0.f;
    if (active && a.gg) {   // per-sample channel gradients for the channel-parallel scatter kernel: gg[i][4*(2a+h)+c]
#pragma unroll
        for (int a6 = 0; a6 < 6; ++a6) {
            const int s0 = 4 * a6;
            *reinterpret_cast<float4*>(a.gg + (size_t)i * 48 + 4 * (2 * a6 + h)) =
                make_float4(gg[s0 >> 4][s0 & 15], gg[s0 >> 4][(s0 & 15) + 1], gg[s0 >> 4][(s0 & 15) + 2], gg[s0 >> 4][(s0 & 15) + 3]);
        }
    }
    if (!a.plane_tail) {   // the plane part of the coordinate gradient is added by k_og<48, true> (scatter.hip) when it is needed at all
        if (active && h == 0) a.gxw[n] = make_float4(gpts[0], gpts[1], gpts[2], 0.f);
        return;
    }
    float4 q = active ? a.xw[n] : zero4();
    Bl b[6];
    plane_setups(f, q.x, q.y, q.z, SCHED_TN(a), b);
    float gx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int a6 = 0; a6 < 6; ++a6) {
        const int q4 = 2 * a6 + h;
        const float4 gq = make_float4(scr[(4 * a6) * 256 + threadIdx.x], scr[(4 * a6 + 1) * 256 + threadIdx.x],
                                      scr[(4 * a6 + 2) * 256 + threadIdx.x], scr[(4 * a6 + 3) * 256 + threadIdx.x]);
        float4 v[6];
        v[0] = bl_sample4(f.aps[0], f.Ca, b[0], q4); v[1] = bl_sample4(f.aps[1], f.Ca, b[1], q4); v[2] = bl_sample4(f.aps[2], f.Ca, b[2], q4);
        v[3] = bl_sample4(f.apt[0], f.Ca, b[3], q4); v[4] = bl_sample4(f.apt[1], f.Ca, b[4], q4); v[5] = bl_sample4(f.apt[2], f.Ca, b[5], q4);
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            float4 o = gq;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (k != p) { o.x *= v[k].x; o.y *= v[k].y; o.z *= v[k].z; o.w *= v[k].w; }
            const float* pl = p == 0 ? f.aps[0] : p == 1 ? f.aps[1] : p == 2 ? f.aps[2] : p == 3 ? f.apt[0] : p == 4 ? f.apt[1] : f.apt[2];
            float* gp = p == 0 ? a.g.aps[0] : p == 1 ? a.g.aps[1] : p == 2 ? a.g.aps[2] : p == 3 ? a.g.apt[0] : p == 4 ? a.g.apt[1] : a.g.apt[2];
            bl_backward4(pl, (active && !a.gg) ? gp : nullptr, f.Ca, b[p], q4, o, gx[p], gy[p]);
        }
    }
    float g3[3] = {0.f, 0.f, 0.f};
    {
        float mx, my;
        plane_mults(f, 0, mx, my); g3[0] += gx[0] * mx; g3[1] += gy[0] * my;
        plane_mults(f, 1, mx, my); g3[0] += gx[1] * mx; g3[2] += gy[1] * my;
        plane_mults(f, 2, mx, my); g3[1] += gx[2] * mx; g3[2] += gy[2] * my;
        plane_mults(f, 3, mx, my); g3[2] += gx[3] * mx;
        plane_mults(f, 4, mx, my); g3[1] += gx[4] * mx;
        plane_mults(f, 5, mx, my); g3[0] += gx[5] * mx;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g3[c] += __shfl_xor(g3[c], 32);
    if (active && h == 0) a.gxw[n] = make_float4(g3[0] + gpts[0], g3[1] + gpts[1], g3[2] + gpts[2], 0.f);
}

static int ensure_app_attrs() {
    static DeviceOnce once;
    return once.lds(ENGINE_LDS_BYTES, k_app_fwd<true>, k_app_fwd<false>, k_app_bwd);
}
// (Round 3 built and measured a PERSISTENT form of this kernel - the whole 145.5 KB forward image resident in LDS, eight independent waves
//  per CU walking their own tiles with no barrier, bit-identical results: 0.372 ms per step against 0.300 ms for this kernel.  With
//  2 700 tiles on 2 048 waves a third of the waves run two tiles back to back while the rest idle, a wave keeps only 12 taps in flight
//  beside the MLP's registers, and the launch owns the CU.  Dropped)
int launch_app_fwd(const AppArgs& aa, int64_t cap_samples, bool stash, hipStream_t st) {
    const unsigned wgs = (unsigned)((cap_samples + WG_SAMPLES - 1) / WG_SAMPLES);
    if (wgs == 0) return 0;
    if (ensure_app_attrs()) return 1;
    if (stash) hipLaunchKernelGGL(k_app_fwd<true>, dim3(wgs), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, aa);
    else hipLaunchKernelGGL(k_app_fwd<false>, dim3(wgs), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, aa);
    LAUNCHCK();
    return 0;
}
int launch_app_bwd(const AppArgs& aa, int64_t cap_samples, hipStream_t st) {
    if (ensure_app_attrs()) return 1;
    hipLaunchKernelGGL(k_app_bwd, dim3((unsigned)((cap_samples + WG_SAMPLES - 1) / WG_SAMPLES)), dim3(WG_THREADS), ENGINE_LDS_BYTES, st, aa);
    return 0;
}
