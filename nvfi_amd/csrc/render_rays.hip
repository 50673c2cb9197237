// render_rays.hip - the per-ray stages of the render: the head of a call (clear, device-side schedule, origin test), sampling with its
// ordered compact lists, volume weights (raw2alpha), the composite, and the adjoints of the weights and of the density lookup.
// Reference semantics: models/tensorf_base.py:290-314 (sample_ray), models/tensorf_model_utils.py:186-197 (raw2alpha),
// models/tensorf_keyframe.py:641-755 (render_pts).
#include "common.h"
#include "render.h"

// ================================================================ sampling + compaction
__global__ void k_any_inside(nvfi_field_desc f, int64_t R, const float* __restrict__ o, int* flag) {
    // tensorf_base.py:294: ((aabb0 <= o) & (o <= aabb1)).any() over every coordinate of every ray
    bool hit = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < R * 3; i += (int64_t)gridDim.x * blockDim.x) {
        int c = (int)(i % 3);
        float v = o[i];
        if (f.aabb[c] <= v && v <= f.aabb[3 + c]) hit = true;
    }
    if (__any(hit) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__device__ __forceinline__ float alpha_lookup(const nvfi_field_desc& f, float x, float y, float z) {
    // AlphaGridMask.sample_alpha: trilinear, align_corners=True, zeros padding (tensorf_model_utils.py:433-439)
    const int W = f.am_dims[0], H = f.am_dims[1], D = f.am_dims[2];
    float ix = (x + 1.f) * ((float)(W - 1) / 2.f), iy = (y + 1.f) * ((float)(H - 1) / 2.f), iz = (z + 1.f) * ((float)(D - 1) / 2.f);
    float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    float wx = ix - fx, wy = iy - fy, wz = iz - fz;
    fx = fminf(fmaxf(fx, -4.f), W + 2.f); fy = fminf(fmaxf(fy, -4.f), H + 2.f); fz = fminf(fmaxf(fz, -4.f), D + 2.f);
    int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    float s = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                int xi = x0 + dx, yi = y0 + dy, zi = z0 + dz;
                if (xi < 0 || xi >= W || yi < 0 || yi >= H || zi < 0 || zi >= D) continue;
                float w = (dx ? wx : 1.f - wx) * (dy ? wy : 1.f - wy) * (dz ? wz : 1.f - wz);
                s += f.amask[((size_t)zi * H + yi) * W + xi] * w;
            }
    return s;
}

// one wave per ray
__global__ __launch_bounds__(256) void k_sample(SampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const nvfi_field_desc& f = a.f;
    const int S = f.n_samples;
    float o[3] = {a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
    float d[3] = {a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
    const float tmin = ray_tmin(f, *a.inside != 0, o, d);
    const float u = (a.train && a.u) ? a.u[r] : 0.f;
    int cnt = 0, cntr = 0;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        bool ok = false, mv = false;
        if (j < S) {
            float rng = (float)j + u;
            float step = f.step_size * rng;
            float z = tmin + step;
            float p[3], xn[3];
            ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[c] = o[c] + d[c] * z;
                if (f.aabb[c] > p[c] || p[c] > f.aabb[3 + c]) ok = false;
                xn[c] = norm_coord(f, c, p[c]);
            }
            if (ok && f.has_amask && !a.train) ok = alpha_lookup(f, xn[0], xn[1], xn[2]) > 0.f;
            const int64_t n = r * S + j;
            a.xw[n] = make_float4(xn[0], xn[1], xn[2], z);
            a.xpre[n] = XPRE_INVALID;
            a.valid[n] = ok ? 1 : 0;
            // a sample outside the velocity gate never moves (v = 0 there, velocity_field.py:28-33,46-51): the warp skips it
            mv = ok && !gated_out(f, xn[0], xn[1], xn[2]);
            if (a.rflag) a.rflag[n] = mv ? 1 : 0;
        }
        cnt += __popcll(__ballot(ok));
        cntr += __popcll(__ballot(mv));
    }
    if (lane == 0) { a.cnt[r] = cnt; if (a.cnt_r) a.cnt_r[r] = cntr; }
}

// ordered fill of the compact list: list[off[r] + rank] = dense index.  The exclusive scan of the per-group counts rides in the same
// launch: a workgroup (4 groups) sums the counts of every group before its own - n <= a few thousand ints out of L2 - instead of reading
// the result of a separate one-workgroup scan kernel (one launch less per compaction: 3 per render, 2 per PDE call); it also writes
// off[] for its groups (k_final_fwd / k_weights_bwd read the per-ray offsets of the masked list), the last one off[n] and *total_out.
__global__ __launch_bounds__(256) void k_fill(int64_t R, int S, const uint8_t* __restrict__ flags, const int* __restrict__ cnt, int* __restrict__ off,
                                              int* __restrict__ list, int* total_out) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4;
    int s = 0;
    for (int64_t i = threadIdx.x; i < r0; i += 256) s += cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) part[w] = s;
    __syncthreads();
    int base = (part[0] + part[1]) + (part[2] + part[3]);
    const int64_t r = r0 + w;
    for (int k = 0; k < w; ++k) base += (r0 + k < R) ? cnt[r0 + k] : 0;
    if (r >= R) return;
    if (lane == 0) {
        off[r] = base;
        if (r == R - 1) { const int tot = base + cnt[r]; off[R] = tot; *total_out = tot; }
    }
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        bool ok = j < S && flags[r * S + j];
        unsigned long long b = __ballot(ok);
        if (ok) list[base + __popcll(b & ((1ull << lane) - 1ull))] = (int)(r * S + j);
        base += __popcll(b);
    }
}

// ---------------------------------------------------------------- round 5: the same lists without the second (and third) launch
// NVFI_FUSED_LAUNCH (default 1): the producers of the flags place the list entries themselves (look-back, common.h); 0 keeps the
// count + k_fill launches of rounds 1-4.  Same flags, same order: the lists are identical entry for entry.
// k_sample + the two k_fill launches behind it
__global__ __launch_bounds__(256) void k_sample_fill(SampleArgs a) {
    __shared__ int cv[4], cr[4];
    __shared__ unsigned long long excl_sh;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + w;
    const bool ron = r < a.R;
    const nvfi_field_desc& f = a.f;
    const int S = f.n_samples;
    int cnt = 0, cntr = 0;
    if (ron) {
        float o[3] = {a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
        float d[3] = {a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
        const float tmin = ray_tmin(f, *a.inside != 0, o, d);
        const float u = (a.train && a.u) ? a.u[r] : 0.f;
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int j = j0 + lane;
            bool ok = false, mv = false;
            if (j < S) {
                float rng = (float)j + u;
                float step = f.step_size * rng;
                float z = tmin + step;
                float p[3], xn[3];
                ok = true;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[c] = o[c] + d[c] * z;
                    if (f.aabb[c] > p[c] || p[c] > f.aabb[3 + c]) ok = false;
                    xn[c] = norm_coord(f, c, p[c]);
                }
                if (ok && f.has_amask && !a.train) ok = alpha_lookup(f, xn[0], xn[1], xn[2]) > 0.f;
                const int64_t n = r * S + j;
                a.xw[n] = make_float4(xn[0], xn[1], xn[2], z);
                a.xpre[n] = XPRE_INVALID;
                a.valid[n] = ok ? 1 : 0;
                mv = ok && !gated_out(f, xn[0], xn[1], xn[2]);
                if (a.rflag) a.rflag[n] = mv ? 1 : 0;
            }
            cnt += __popcll(__ballot(ok));
            cntr += __popcll(__ballot(mv));
        }
    }
    if (lane == 0) { cv[w] = cnt; cr[w] = cntr; }
    __syncthreads();
    if (w == 0) {
        const unsigned long long agg = ((unsigned long long)((cv[0] + cv[1]) + (cv[2] + cv[3])) << 31) | (unsigned long long)((cr[0] + cr[1]) + (cr[2] + cr[3]));
        const unsigned long long e = lb_exclusive(a.lb, (int)blockIdx.x, agg);
        if (lane == 0) {
            excl_sh = e;
            if (blockIdx.x == gridDim.x - 1) {
                const unsigned long long tot = e + agg;
                *a.total_v = (int)(tot >> 31);
                if (a.rflag) *a.total_r = (int)(tot & 0x7fffffffull);
            }
        }
    }
    __syncthreads();
    if (!ron) return;
    int base_v = (int)(excl_sh >> 31), base_r = (int)(excl_sh & 0x7fffffffull);
    for (int k = 0; k < w; ++k) { base_v += cv[k]; base_r += cr[k]; }
    // (the flags were written by this very lane above)
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool ok = j < S && a.valid[r * S + j];
        const unsigned long long b = __ballot(ok);
        if (ok) a.vlist[base_v + __popcll(b & ((1ull << lane) - 1ull))] = (int)(r * S + j);
        base_v += __popcll(b);
        if (a.rflag) {
            const bool mv = j < S && a.rflag[r * S + j];
            const unsigned long long bm = __ballot(mv);
            if (mv) a.rlist[base_r + __popcll(bm & ((1ull << lane) - 1ull))] = (int)(r * S + j);
            base_r += __popcll(bm);
        }
    }
}

// scan + ordered fill for n_groups groups of 64 flags (used by the PDE prefilter)
int launch_scan_fill(const int* cnt, int* off, int64_t ngroups, int* total, const uint8_t* flags, int* list, hipStream_t st) {
    if (ngroups <= 0) return launch_zero(total, sizeof(int), st);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((ngroups + 3) / 4)), dim3(256), 0, st, ngroups, 64, flags, cnt, off, list, total);
    LAUNCHCK();
    return 0;
}

// ================================================================ density
// (forward: k_density_q in scatter.hip - lanes = sample x channel quad)

// backward: gxpre -> plane grads (atomics) + coordinate grads
__global__ __launch_bounds__(256) void k_density_bwd(DensityArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int count = *a.count;
    if (i >= count) return;
    const nvfi_field_desc& f = a.f;
    const int n = a.list[i];
    const float4 q = a.xw[n];
    const float gf = a.gxpre[n];
    Bl b[6];
    plane_setups(f, q.x, q.y, q.z, SCHED_TN(a), b);
    float gx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* pl[6] = {f.dps[0], f.dps[1], f.dps[2], f.dpt[0], f.dpt[1], f.dpt[2]};
    float* gp[6] = {a.g.dps[0], a.g.dps[1], a.g.dps[2], a.g.dpt[0], a.g.dpt[1], a.g.dpt[2]};
    const int nq = f.Cd >> 2;
    for (int q4 = 0; q4 < nq; ++q4) {
        float4 v[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) v[p] = bl_sample4(pl[p], f.Cd, b[p], q4);
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            float4 o = make_float4(gf, gf, gf, gf);
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (k != p) { o.x *= v[k].x; o.y *= v[k].y; o.z *= v[k].z; o.w *= v[k].w; }
            bl_backward4(pl[p], gp[p], f.Cd, b[p], q4, o, gx[p], gy[p]);
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
    if (a.gxk) {
        float4 ga = a.mflag[n] ? a.gxw[n] : zero4();   // appearance-branch part (masked samples only)
        a.gxk[n] = make_float4(ga.x + g3[0], ga.y + g3[1], ga.z + g3[2], 0.f);   // dense (per sample): the RK2 adjoint walks its own list
    }
}

// ================================================================ volume weights (raw2alpha) + composites
// one wave per ray; 64-sample segments with a carried transmittance
// SEL (nvfi_render_fwd_select): sigma' = sigma * s(x).  A sample that is not valid has sigma == 0 exactly (XPRE_INVALID) and no s: it stays 0
template <bool SEL>
__global__ __launch_bounds__(256) void k_weights_fwd(WeightArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int S = a.S;
    float carry = 1.f, accs = 0.f, dep = 0.f;
    int cnt = 0;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < S;
        const int64_t n = r * S + j;
        float sig = 0.f, dist = 0.f, z = 0.f;
        if (in) {
            sig = softplus_f(a.xpre[n]);
            if (SEL) sig = sig > 0.f ? sig * a.sel[n] : 0.f;
            z = a.xw[n].w;
            if (j + 1 < S) dist = (a.xw[n + 1].w - z) * a.distance_scale;
        }
        const float al = 1.f - expf(-sig * dist);
        const float fct = 1.f - al + 1e-10f;
        float p = fct;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { float t = __shfl_up(p, o); if (lane >= o) p *= t; }
        float ex = __shfl_up(p, 1);
        if (lane == 0) ex = 1.f;
        const float T = carry * ex;
        const float w = al * T;
        carry = carry * __shfl(p, 63);
        const bool m = in && w > a.weight_thres;
        if (in) { a.weight[n] = w; a.mflag[n] = m ? 1 : 0; accs += w; dep += w * z; }
        cnt += __popcll(__ballot(m));
    }
    accs = wave_sum(accs); dep = wave_sum(dep);
    if (lane == 0) {
        a.acc[r] = accs;
        a.depth[r] = dep + (1.f - accs) * a.far_;
        a.cnt_m[r] = cnt;
    }
}

// the call's counters for the caller (device-side totals -> int64[8]); by k_counters, or by workgroup 0 of k_final_fwd (round 5)
__device__ __forceinline__ void counters_body(const int* c, int nsteps, int64_t* out, const float* sched) {
    out[0] = c[0];
    out[1] = nsteps > 0 ? c[3] : 0;
    out[2] = c[1];
    out[3] = (int64_t)(nsteps > 0 ? c[3] : 0) * 2 * nsteps;
    out[4] = out[5] = out[6] = 0;
    out[7] = sched ? __float_as_int(sched[3]) : 0;      // 1: the device-side time did not fit the planned RK2 step count (the planned time was rendered)
}

// k_weights_fwd + the k_fill launch behind it: the ordered list of appearance-masked samples (weight > rayMarch_weight_thres) and the per-ray
// offsets into it (k_final_fwd / k_weights_bwd read off_m) from the same launch
template <bool SEL>
__global__ __launch_bounds__(256) void k_weights_fill(WeightArgs a) {
    __shared__ int cm[4];
    __shared__ unsigned long long excl_sh;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + w;
    const bool ron = r < a.R;
    const int S = a.S;
    int cnt = 0;
    if (ron) {
        float carry = 1.f, accs = 0.f, dep = 0.f;
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < S;
            const int64_t n = r * S + j;
            float sig = 0.f, dist = 0.f, z = 0.f;
            if (in) {
                sig = softplus_f(a.xpre[n]);
                if (SEL) sig = sig > 0.f ? sig * a.sel[n] : 0.f;
                z = a.xw[n].w;
                if (j + 1 < S) dist = (a.xw[n + 1].w - z) * a.distance_scale;
            }
            const float al = 1.f - expf(-sig * dist);
            const float fct = 1.f - al + 1e-10f;
            float p = fct;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { float t = __shfl_up(p, o); if (lane >= o) p *= t; }
            float ex = __shfl_up(p, 1);
            if (lane == 0) ex = 1.f;
            const float T = carry * ex;
            const float wgt = al * T;
            carry = carry * __shfl(p, 63);
            const bool m = in && wgt > a.weight_thres;
            if (in) { a.weight[n] = wgt; a.mflag[n] = m ? 1 : 0; accs += wgt; dep += wgt * z; }
            cnt += __popcll(__ballot(m));
        }
        accs = wave_sum(accs); dep = wave_sum(dep);
        if (lane == 0) {
            a.acc[r] = accs;
            a.depth[r] = dep + (1.f - accs) * a.far_;
        }
    }
    if (lane == 0) cm[w] = cnt;
    __syncthreads();
    if (w == 0) {
        const unsigned long long agg = (unsigned long long)((cm[0] + cm[1]) + (cm[2] + cm[3]));
        const unsigned long long e = lb_exclusive(a.lb, (int)blockIdx.x, agg);
        if (lane == 0) {
            excl_sh = e;
            if (blockIdx.x == gridDim.x - 1) { const int tot = (int)(e + agg); a.off_m_out[a.R] = tot; *a.total_m = tot; }
        }
    }
    __syncthreads();
    if (!ron) return;
    int base = (int)excl_sh;
    for (int k = 0; k < w; ++k) base += cm[k];
    if (lane == 0) a.off_m_out[r] = base;
    for (int j0 = 0; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool ok = j < S && a.mflag[r * S + j];
        const unsigned long long b = __ballot(ok);
        if (ok) a.mlist[base + __popcll(b & ((1ull << lane) - 1ull))] = (int)(r * S + j);
        base += __popcll(b);
    }
}

__global__ __launch_bounds__(256) void k_final_fwd(FinalArgs a) {
    __shared__ float red[4];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    const bool ron = r < a.R;
    float se = 0.f;
    if (ron) {
        const int b0 = a.off_m[r], b1 = a.off_m[r + 1];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        for (int i = b0 + lane; i < b1; i += 64) {
            const float w = a.weight[a.mlist[i]];
            const float4 c = a.rgbs[i];
            c0 += w * c.x; c1 += w * c.y; c2 += w * c.z;
        }
        c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
        if (lane == 0) {
            if (a.white_bg) { float bg = 1.f - a.acc[r]; c0 += bg; c1 += bg; c2 += bg; }
            a.rgb_pre[r] = make_float4(c0, c1, c2, 0.f);
            const float o0 = fminf(fmaxf(c0, 0.f), 1.f), o1 = fminf(fmaxf(c1, 0.f), 1.f), o2 = fminf(fmaxf(c2, 0.f), 1.f);
            a.rgb[3 * r] = o0; a.rgb[3 * r + 1] = o1; a.rgb[3 * r + 2] = o2;
            if (a.target) {
                const float inv = 1.f / (float)(3 * a.R);
                const float d0 = o0 - a.target[3 * r], d1 = o1 - a.target[3 * r + 1], d2 = o2 - a.target[3 * r + 2];
                a.g_rgb_out[3 * r] = a.loss_scale * (2.f * d0 * inv); a.g_rgb_out[3 * r + 1] = a.loss_scale * (2.f * d1 * inv); a.g_rgb_out[3 * r + 2] = a.loss_scale * (2.f * d2 * inv);
                se = (d0 * d0 + d1 * d1) + d2 * d2;
            }
        }
    }
    if (a.counters_out && blockIdx.x == 0 && threadIdx.x == 0) counters_body(a.c, a.nsteps, a.counters_out, a.sched);
    if (!a.target) return;
    if (lane == 0) red[wv] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(a.partial + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && wv == 0) {      // the last workgroup sums the partials in workgroup order: the value does not depend on which one that is
        float t = 0.f;
        for (int k = lane; k < (int)gridDim.x; k += 64) t += __hip_atomic_load(a.partial + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = wave_sum(t);
        if (lane == 0) { *a.loss_out = t * (1.f / (float)(3 * a.R)); *a.ticket = 0; }
    }
}

// backward of composites + raw2alpha: produces d/d(xpre) per sample
__global__ __launch_bounds__(256) void k_weights_bwd(WeightArgs a) {
    __shared__ float carries[4][17];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= a.R) return;
    const int S = a.S;
    const int nseg = (S + 63) >> 6;
    // upstream
    float gr[3] = {0.f, 0.f, 0.f};
    if (a.g_rgb) {
        const float4 pre = a.rgb_pre[r];
        const float pv[3] = {pre.x, pre.y, pre.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) gr[c] = (pv[c] >= 0.f && pv[c] <= 1.f) ? a.g_rgb[3 * r + c] : 0.f;
    }
    const float gd = a.g_depth ? a.g_depth[r] : 0.f, ga = a.g_acc ? a.g_acc[r] : 0.f;
    const float bgsum = a.white_bg ? (gr[0] + gr[1] + gr[2]) : 0.f;
    // pass 1: carried transmittance at the start of each segment
    float carry = 1.f;
    for (int sg = 0; sg < nseg; ++sg) {
        const int j = sg * 64 + lane;
        const int64_t n = r * S + j;
        float sig = 0.f, dist = 0.f;
        if (j < S) {
            sig = softplus_f(a.xpre[n]);
            if (j + 1 < S) dist = (a.xw[n + 1].w - a.xw[n].w) * a.distance_scale;
        }
        const float al = 1.f - expf(-sig * dist);
        float p = 1.f - al + 1e-10f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { float t = __shfl_up(p, o); if (lane >= o) p *= t; }
        if (lane == 0) carries[wv][sg] = carry;
        carry = carry * __shfl(p, 63);
    }
    // pass 2: reverse segments
    float suffix = 0.f;   // sum_{i>j} gw_i w_i over later segments
    int mrank_end = a.off_m[r + 1];
    for (int sg = nseg - 1; sg >= 0; --sg) {
        const int j = sg * 64 + lane;
        const bool in = j < S;
        const int64_t n = r * S + j;
        float sig = 0.f, dist = 0.f, z = 0.f, xp = XPRE_INVALID;
        bool m = false;
        if (in) {
            xp = a.xpre[n];
            sig = softplus_f(xp);
            z = a.xw[n].w;
            if (j + 1 < S) dist = (a.xw[n + 1].w - z) * a.distance_scale;
            m = a.mflag[n] != 0;
        }
        const float al = 1.f - expf(-sig * dist);
        const float fct = 1.f - al + 1e-10f;
        float p = fct;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { float t = __shfl_up(p, o); if (lane >= o) p *= t; }
        float ex = __shfl_up(p, 1);
        if (lane == 0) ex = 1.f;
        const float T = carries[wv][sg] * ex;
        const float w = al * T;
        // colour of masked samples comes from the compact list (ray-ordered)
        const unsigned long long mb = __ballot(m);
        const int seg_cnt = __popcll(mb);
        float gw = -bgsum + ga + gd * (z - a.far_) + ((a.g_weight && in) ? a.g_weight[n] : 0.f);
        if (m) {
            const int mi = mrank_end - seg_cnt + __popcll(mb & ((1ull << lane) - 1ull));
            const float4 c = a.rgbs[mi];
            gw += gr[0] * c.x + gr[1] * c.y + gr[2] * c.z;
        }
        mrank_end -= seg_cnt;
        if (!in) gw = 0.f;
        // suffix sums within the segment: s_j = sum_{i>j} gw_i w_i
        float v = gw * w, inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { float t = __shfl_down(inc, o); if (lane + o < 64) inc += t; }
        const float suf = suffix + (inc - v);
        suffix = suffix + __shfl(inc, 0);
        if (in) {
            const float galpha = gw * T - suf / fct;
            const float gsig = galpha * dist * (1.f - al);
            a.gxpre[n] = gsig * (xp > 20.f ? 1.f : sigmoid_f(xp));
        }
    }
}

// Device-side schedule (hipGraph replay): rk_schedule / norm_time / time_row0 (common.h), the host's own functions, on a time held in device
// memory.  The launch plan (number of RK2 steps -> which kernels run, stash sizes) was fixed on the host from `t_plan`;
// if the device time implies a different step count the record falls back to the plan's schedule and raises sched[3] (mirrored into
// counters[7] by k_counters) - results are then those of t_plan, never undefined.
__device__ void sched_body(const SchedArgs& a) {
    const nvfi_field_desc& f = a.f;
    float* S = a.sched;
    const float t = *a.t_dev;
    float base;
    int n = rk_schedule(f, t, a.flags, &base, S + SCHED_DT, S + SCHED_TC);
    float tn = f.use_vel ? norm_time(f, base) : norm_time(f, t);
    const bool bad = n != a.nsteps_plan;      // (-1: more steps than the record holds)
    if (bad) {                                // not the planned launch shape: render the planned time instead, and say so
        n = a.nsteps_plan;
        for (int s = 0; s < n && s < 4; ++s) { S[SCHED_DT + s] = a.dt_plan[s]; S[SCHED_TC + s] = a.tc_plan[s]; }
        tn = a.tn_plan;
    }
    S[0] = tn; S[1] = __int_as_float(time_row0(f, tn)); S[2] = __int_as_float(n); S[3] = __int_as_float(bad ? 1 : 0);
}
__global__ void k_sched(SchedArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    sched_body(a);
}

// The head of a render call in ONE workgroup: clears the call's counters / sort histograms / look-back words (the forward's memset), derives the
// device-side schedule when the frame time lives in device memory (k_sched), and tests the ray origins against the box (k_any_inside,
// tensorf_base.py:294).  Used for R <= PROLOGUE_MAX_RAYS; larger calls keep the three launches.
#define PROLOGUE_MAX_RAYS 8192
struct PrologueArgs { SchedArgs sc; int do_sched; int64_t R; const float* o; int* zero_from; int64_t zero_ints; int* inside; };
__global__ __launch_bounds__(256) void k_prologue(PrologueArgs a) {
    __shared__ int hit_any;
    if (threadIdx.x == 0) hit_any = 0;
    int4* z4 = reinterpret_cast<int4*>(a.zero_from);         // (256-byte aligned, a multiple of 256 bytes)
    for (int64_t k = threadIdx.x; k < a.zero_ints / 4; k += 256) z4[k] = make_int4(0, 0, 0, 0);
    __syncthreads();
    const nvfi_field_desc& f = a.sc.f;
    bool hit = false;
    for (int64_t i = threadIdx.x; i < a.R * 3; i += 256) {
        const int c = (int)(i % 3);
        const float v = a.o[i];
        if (f.aabb[c] <= v && v <= f.aabb[3 + c]) hit = true;
    }
    if (__any(hit) && (threadIdx.x & 63) == 0) hit_any = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        *a.inside = hit_any;       // (inside the zeroed range: written after the clear, by the same workgroup)
        if (a.do_sched) sched_body(a.sc);
    }
}

__global__ void k_counters(const int* c, int nsteps, int64_t* out, const float* sched) {
    if (threadIdx.x == 0) counters_body(c, nsteps, out, sched);
}

// ================================================================ launchers
// head of a forward: sc.f is the field; sc.t_dev != NULL asks for the device-side schedule (the rest of sc: the host's plan)
int launch_ray_head(const SchedArgs& sc, int64_t R, const float* rays_o, int* zero_from, int64_t zero_bytes, int* inside, bool fused, hipStream_t st) {
    if (fused && R <= PROLOGUE_MAX_RAYS) {      // one-workgroup prologue: clear + schedule + origin test
        PrologueArgs pa; memset(&pa, 0, sizeof(pa));
        pa.sc = sc; pa.do_sched = sc.t_dev ? 1 : 0; pa.R = R; pa.o = rays_o; pa.zero_from = zero_from; pa.zero_ints = zero_bytes / 4; pa.inside = inside;
        hipLaunchKernelGGL(k_prologue, dim3(1), dim3(256), 0, st, pa);
    } else {
        if (launch_zero(zero_from, zero_bytes, st)) return 1;
        if (sc.t_dev) hipLaunchKernelGGL(k_sched, dim3(1), dim3(64), 0, st, sc);
        hipLaunchKernelGGL(k_any_inside, dim3(64), dim3(256), 0, st, sc.f, R, rays_o, inside);
    }
    LAUNCHCK();
    return 0;
}
// sampling + the ordered lists of the valid samples and (sa.rflag) of those inside the velocity gate; off_v / off_r: the unfused form's scans
int launch_sample(const SampleArgs& sa, int* off_v, int* off_r, bool fused, hipStream_t st) {
    const dim3 grid((unsigned)((sa.R + 3) / 4));
    if (fused) hipLaunchKernelGGL(k_sample_fill, grid, dim3(256), 0, st, sa);
    else {
        hipLaunchKernelGGL(k_sample, grid, dim3(256), 0, st, sa);
        hipLaunchKernelGGL(k_fill, grid, dim3(256), 0, st, sa.R, sa.f.n_samples, sa.valid, sa.cnt, off_v, sa.vlist, sa.total_v);
        if (sa.rflag) hipLaunchKernelGGL(k_fill, grid, dim3(256), 0, st, sa.R, sa.f.n_samples, sa.rflag, sa.cnt_r, off_r, sa.rlist, sa.total_r);
    }
    LAUNCHCK();
    return 0;
}
// weights + the ordered list of the appearance-masked samples; wa.sel: the object-selected form
int launch_weights_fwd(const WeightArgs& wa, bool fused, hipStream_t st) {
    const dim3 grid((unsigned)((wa.R + 3) / 4));
    if (fused) {
        if (wa.sel) hipLaunchKernelGGL(k_weights_fill<true>, grid, dim3(256), 0, st, wa);
        else hipLaunchKernelGGL(k_weights_fill<false>, grid, dim3(256), 0, st, wa);
    } else {
        if (wa.sel) hipLaunchKernelGGL(k_weights_fwd<true>, grid, dim3(256), 0, st, wa);
        else hipLaunchKernelGGL(k_weights_fwd<false>, grid, dim3(256), 0, st, wa);
        hipLaunchKernelGGL(k_fill, grid, dim3(256), 0, st, wa.R, wa.S, wa.mflag, wa.cnt_m, wa.off_m_out, wa.mlist, wa.total_m);
    }
    LAUNCHCK();
    return 0;
}
// composite; the call's counters for the caller ride in the same launch (fused) or take k_counters
int launch_final_fwd(FinalArgs fa, int64_t* counters, bool fused, hipStream_t st) {
    fa.counters_out = fused ? counters : nullptr;
    hipLaunchKernelGGL(k_final_fwd, dim3((unsigned)((fa.R + 3) / 4)), dim3(256), 0, st, fa);
    if (counters && !fused) hipLaunchKernelGGL(k_counters, dim3(1), dim3(64), 0, st, fa.c, fa.nsteps, counters, fa.sched);
    LAUNCHCK();
    return 0;
}
int launch_weights_bwd(const WeightArgs& wa, hipStream_t st) {
    hipLaunchKernelGGL(k_weights_bwd, dim3((unsigned)((wa.R + 3) / 4)), dim3(256), 0, st, wa);
    LAUNCHCK();
    return 0;
}
int launch_density_bwd(const DensityArgs& da, int64_t N, hipStream_t st) {
    hipLaunchKernelGGL(k_density_bwd, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, da);
    LAUNCHCK();
    return 0;
}
