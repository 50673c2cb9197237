// frags.hip - every packed weight image of a field: nvfi_frag_cache_bytes / nvfi_pack_frags (all of them in one launch into the field's
// cache) and vel_images (a host entry point's way to the velocity net's images, cached or packed into its own workspace; frags.h).
// Reference counterpart: none - the reference's nn.Linear weights are read by ATen as they are (models/velocity_field.py:60-67,
// models/tensorf_base.py:67-98); this is the MFMA operand layout of those weights.
#include <string.h>
#include "common.h"
#include "frags.h"

// ---------------------------------------------------------------- layouts
struct FragCache { float *render, *vel, *anet, *vel_x4f, *vel_x4b, *a_x4b; void* vel_x6; void* vel_x6t; int64_t total; };
static void frag_cache_layout(const float* base, FragCache* c) {
    Bump B{(char*)base, 0, 0};
    c->render = B.take<float>(RENDER_FRAG_FLOATS);
    c->vel = B.take<float>(VEL_FRAG_FLOATS);
    c->anet = B.take<float>(VEL_FRAG_FLOATS);
    c->vel_x4f = B.take<float>(VEL_X4F_FLOATS);
    c->vel_x4b = B.take<float>(VEL_X4B_FLOATS);
    c->a_x4b = B.take<float>(A_X4B_FLOATS);
    c->vel_x6 = B.take<float>(X6_IMAGE_BYTES / 4);         // the three bfloat16 images of weight_net's layers 0..4 (vel_x6.hip)
    c->vel_x6t = B.take<float>(X6_IMAGE_BYTES / 4);        // ... and of their transposes (round 6: the dgrad of vel_fuse.hip on x6)
    c->total = align_up(B.off, 256);
}
// The x4 sets, each stated once: {layer, 32-row tiles, K steps} in buffer order.  Forward: f[0] (4 tiles x 14 steps), f[1..4], f[5] (1 x 64);
// transposed: T0 (1 tile x 64 steps), t[1..4], t[5] (4 tiles x 4 steps); a_weight_net's transposed set has no T0 (pde_fuse.hip reads t[1..5])
struct X4Slot { int l, MT, NS; };
struct X4Set { X4Slot s[6]; int n; };
static constexpr X4Set X4F_SET = {{{0, 4, 14}, {1, 4, 64}, {2, 4, 64}, {3, 4, 64}, {4, 4, 64}, {5, 1, 64}}, 6};
static constexpr X4Set X4B_SET = {{{0, 1, 64}, {1, 4, 64}, {2, 4, 64}, {3, 4, 64}, {4, 4, 64}, {5, 4, 4}}, 6};
static constexpr X4Set A_X4B_SET = {{{1, 4, 64}, {2, 4, 64}, {3, 4, 64}, {4, 4, 64}, {5, 4, 4}}, 5};
static constexpr int x4_set_floats(const X4Set& S) { int n = 0; for (int i = 0; i < S.n; ++i) n += X4_FLOATS(S.s[i].MT, S.s[i].NS); return n; }
static_assert(x4_set_floats(X4F_SET) == VEL_X4F_FLOATS && x4_set_floats(X4B_SET) == VEL_X4B_FLOATS && x4_set_floats(A_X4B_SET) == A_X4B_FLOATS,
              "the x4 buffer sizes of the plans (pde.h) are the sets' sizes");
// pointer form: p4[l] for the layers of the set (the rest NULL); job form, with xj: the k_frag_x4 jobs that make it from plain fragments frag[l]
static void x4_set(const X4Set& S, const float* const* frag, float* buf, const float4** p4, X4Jobs* xj) {
    for (int l = 0; l < 6; ++l) p4[l] = nullptr;
    for (int i = 0; i < S.n; ++i) {
        const X4Slot& s = S.s[i];
        p4[s.l] = reinterpret_cast<const float4*>(buf);
        if (xj) { xj->src[xj->n] = frag[s.l]; xj->dst[xj->n] = buf; xj->MT[xj->n] = s.MT; xj->NS[xj->n] = s.NS; ++xj->n; }
        buf += X4_FLOATS(s.MT, s.NS);
    }
}

extern "C" int nvfi_frag_cache_bytes(const nvfi_field_desc* f, int64_t* bytes) {
    (void)f;
    FragCache c; frag_cache_layout(nullptr, &c);
    *bytes = c.total;
    return 0;
}

extern "C" int nvfi_pack_frags(const nvfi_field_desc* f, void* cache, int64_t cache_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!cache) return nvfi_fail(2, "nvfi_pack_frags: cache is NULL");
    FragCache c; frag_cache_layout((const float*)cache, &c);
    if (c.total > cache_bytes) return nvfi_fail(4, "fragment cache too small: need %lld bytes, got %lld", (long long)c.total, (long long)cache_bytes);
    // the plain fragment sets, through the job builders of the per-call path (same layouts, same kernels' index maps) ...
    PackJobs tmp; tmp.n = 0;
    PackJobsAll all; memset(&all, 0, sizeof(all));
    auto take = [&]() { for (int i = 0; i < tmp.n; ++i) all.j[all.n++] = tmp.j[i]; tmp.n = 0; };
    RenderFrags RW; VelFrags VW, AW;
    memset(&VW, 0, sizeof(VW)); memset(&AW, 0, sizeof(AW));
    if (pack_render_frags(f, c.render, &RW, &tmp)) return 3;
    take();
    if (f->use_vel) {
        if (pack_vel_frags(f->vW, f->vb, c.vel, &VW, &tmp)) return 3;
        take();
        if (pack_vel_frags(f->aW, f->ab, c.anet, &AW, &tmp)) return 3;
        take();
        // ... and the x4 copies straight from the weights: the job of the plain fragment with x4 = 1 and the x4 destination
        int rc = 0;
        auto add_x4 = [&](const X4Set& S, const float* const* frag, float* buf) {
            X4Jobs xj; xj.n = 0; const float4* p4[6];
            x4_set(S, frag, buf, p4, &xj);
            for (int k = 0; k < xj.n; ++k) {
                const PackJob* src = nullptr;
                for (int i = 0; i < all.n && !src; ++i) if (all.j[i].frag == xj.src[k] && !all.j[i].x4) src = &all.j[i];
                if (!src || all.n >= MAX_PACK_JOBS_ALL) { rc = 1; return; }
                PackJob J = *src;
                J.frag = xj.dst[k]; J.bfrag = nullptr; J.b = nullptr; J.x4 = 1;
                all.j[all.n++] = J;
            }
        };
        add_x4(X4F_SET, VW.f, c.vel_x4f); add_x4(X4B_SET, VW.t, c.vel_x4b); add_x4(A_X4B_SET, AW.t, c.a_x4b);
        if (rc) return nvfi_fail(3, "nvfi_pack_frags: job table");
    }
    X6PackArgs x6; memset(&x6, 0, sizeof(x6));
    if (f->use_vel) { for (int l = 0; l < 5; ++l) x6.W[l] = f->vW[l]; x6.img = reinterpret_cast<b8_t*>(c.vel_x6); x6.imgT = reinterpret_cast<b8_t*>(c.vel_x6t); }
    return launch_pack_all(all, f->use_vel ? &x6 : nullptr, st);
}

// ---------------------------------------------------------------- the resolver
float* render_frag_room(const nvfi_field_desc* f, float* own) {
    if (!f->frags) return own;
    FragCache c; frag_cache_layout(f->frags, &c);
    return c.render;
}

int vel_images(const nvfi_field_desc* f, unsigned need, const VelImageRoom& room, VelImages* out, const PackJobs* ride, unsigned have, hipStream_t st) {
    memset(out, 0, sizeof(*out));
    VelImageRoom at = room;
    const bool cached = f->frags != nullptr;
    if (cached) {
        FragCache c; frag_cache_layout(f->frags, &c);
        at = VelImageRoom{c.vel, c.anet, c.vel_x4f, c.vel_x4b, c.a_x4b, c.vel_x6, c.vel_x6t};
        have = ~0u;
    }
    if (need & VI_X6T) need |= VI_X6;       // (one pack launch writes the image and its transpose)
    static const char* const names[7] = {"weight_net fragments", "a_weight_net fragments", "x4 forward fragments", "x4 transposed fragments",
                                         "x4 transposed fragments of a_weight_net", "x6 image", "transposed x6 image"};      // (in the order of the VI_ bits)
    const void* const rooms[7] = {at.vel, at.anet, at.x4f, at.x4b, at.a_x4b, at.x6, at.x6t};
    for (int i = 0; i < 7; ++i)
        if ((need >> i & 1) && !rooms[i]) return nvfi_fail(3, "vel_images: the call's plan has no room for the %s", names[i]);
    // pointers of everything needed; jobs of what the room does not hold yet
    PackJobs jobs, held[2]; jobs.n = held[0].n = held[1].n = 0;
    if (ride && !cached) jobs = *ride;
    if ((need & VI_VEL) && pack_vel_frags(f->vW, f->vb, at.vel, &out->VW, (have & VI_VEL) ? &held[0] : &jobs)) return 3;
    if ((need & VI_ANET) && pack_vel_frags(f->aW, f->ab, at.anet, &out->AW, (have & VI_ANET) ? &held[1] : &jobs)) return 3;
    X4Jobs xv, xa; xv.n = xa.n = 0;
    if (((need & ~have & (VI_X4F | VI_X4B)) && !(need & VI_VEL)) || ((need & ~have & VI_A_X4B) && !(need & VI_ANET)))
        return nvfi_fail(3, "vel_images: x4 copies are packed from their net's plain fragments, which the call did not ask for");
    if (need & VI_X4F) x4_set(X4F_SET, out->VW.f, at.x4f, out->f4, (have & VI_X4F) ? nullptr : &xv);
    if (need & VI_X4B) x4_set(X4B_SET, out->VW.t, at.x4b, out->t4, (have & VI_X4B) ? nullptr : &xv);
    if (need & VI_A_X4B) x4_set(A_X4B_SET, out->AW.t, at.a_x4b, out->ta4, (have & VI_A_X4B) ? nullptr : &xa);
    if (need & VI_X6) out->x6 = at.x6;
    if (need & VI_X6T) out->x6t = at.x6t;
    if (cached) return 0;
    if (jobs.n && launch_pack(jobs, st)) return 1;
    if (launch_frag_x4(xv, st) || launch_frag_x4(xa, st)) return 1;
    if ((need & ~have & (VI_X6 | VI_X6T)) && launch_pack_x6(f->vW, at.x6, st, (need & VI_X6T) ? at.x6t : nullptr)) return 1;
    return 0;
}
