"""The object branches of an eval-mode render on the device (objects.hip: nvfi_render_objects, k_select_fwd behind nvfi_render_fwd_select;
TensorVMKeyframeTimeKplane.render_objects, Renderer.render_objects) against their float64 restatement (tests/objects64.py, pinned to the reference
by tests/test_objects_golden.py), fields A and B with the fixture's MaskField (K = 8 and 3; K = 5: the first five rows of the K = 8 head; K = 9, 17
and 32 on field A: the fixture's trunk under the heads of tests/maskfield64.py's params_for - from K = 9 on, accumulator registers 4..15 of the
logit tile of k_mask_fwd and k_select_fwd carry live rows, from K = 17 on both half-waves hold rows >= 8).

Layers: the yardstick is fed the DEVICE's own weight map, so the masked list is the same on both sides.  Bound per map, relative to max |map|:
4 x the plain-fp32 floor of the case - objects64(float32) against objects64(float64) on the same weights, measured on the CPU, never below one fp32
ulp of the map scale (objects64.layer_floor); for the golden cases objects64.GOLDEN_FLOOR.  The factor 4 is the margin of the project's other
yardstick tests for the rounding-order freedom of an MFMA sum against a sequential one.
obj_acc is compared with mask_map bit for bit: k_obj_final adds in k_mask_final's order.
Selected renders: rgb, depth, acc, weight by the rule of tests/test_gpu_render64.py (objects64.MAP_RTOL x |ref| + helpers.FP32_FLOOR element-wise);
rays with a sample in the yardstick's near-threshold report (float64 or float32 run) may be set aside, at most 2 % of the case's rays.
Occlusion: with object k removed, s_j = 1 - m_jk, and per sample w'_j = alpha'_j T'_j >= s_j alpha_j T_j = s_j w_j: T' >= T (less density in
front never lowers the transmittance behind it) and alpha' = 1 - exp(-s sigma dist) >= s (1 - exp(-sigma dist)) by concavity.  The layers of the
selected render weigh w'_j with the same softmax, so the remaining objects hold sum_j w'_j s_j >= sum_j w_j s_j^2 = [their acc in the full render]
- sum_j w_j s_j (1 - s_j).  The bound of "the acc of the remaining objects' layers is >= their acc in the full render, minus the bound" is
therefore, per ray: that softness term (from the device's full-render weights and the yardstick's float64 s_j; it vanishes for hard masks, where
s_j is 0 or 1) + weight_thres for every sample that is appearance-masked in the full render and not in the selected one (it leaves the layer sums
and carried s_j w_j <= w'_j <= thres) + rounding (4 x the layer floor of the map scale per remaining object, and objects64.MAP_RTOL x the sum +
helpers.FP32_FLOOR["acc"] for the device's w').  A first version of this test left the softness term out and asked for sum_j w'_j s_j >= sum_j w_j
s_j: false for soft masks - the float64 yardstick itself gives -0.132 on field A (fixture masks: mean max_k m = 0.59) and -0.098 on field B,
the figures the device gave.  The sharp statement needs no softness term and is asserted too: the acc of the selected render, sum_j w'_j, is >=
the remaining objects' layer acc in the full render minus rounding.  That something is revealed is asserted on the weights: some sample carries
more than 1e-3 more weight than in the full render."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import maskfield64 as m64
import objects64 as o64
import render64 as r64
from conftest import GOLD
from helpers import FP32_FLOOR, field_state, make_model
from test_objects_golden import mask_state

pytestmark = pytest.mark.gpu
T_NONKEY = 19.0 / 60.0


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "objects.npz"))


K_WIDE = (9, 17, 32)


def _mask_field(sd, K):
    from nvfi_amd.models import MaskField
    mf = MaskField(n_layer=4, n_dim=128, input_dim=3, skips=[], mask_dim=K, mask_act="softmax")
    own = mf.state_dict()
    if K > 8:       # the fixture's trunk under a head of maskfield64.params_for
        sd = dict(sd, **{"mask_fc.weight": m64.params_for(K)[8], "mask_fc.bias": m64.params_for(K)[9]})
    for k, v in sd.items():
        own[k].copy_(torch.from_numpy(np.ascontiguousarray(v[:K] if k.startswith("mask_fc") else v)))
    return mf.cuda().eval()


@pytest.fixture(scope="module")
def ctx(gold, fx):
    out = {}
    for kind in "AB":
        model, meta = make_model(kind)
        model.eval()
        sd = mask_state(fx, kind)
        mfs = {K: _mask_field(sd, K) for K in ((8, 5) + K_WIDE if kind == "A" else (3,))}
        out[kind] = dict(model=model, f=model.nvfi, field=r64.Field(*field_state(model)), o=gold[f"{kind}:rays_o"], d=gold[f"{kind}:rays_d"],
                         white=bool(meta["white_background"]), mfs=mfs, K0=8 if kind == "A" else 3)
    yield out
    for c in out.values():
        c["f"].mask_field = None


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(c, o, d, t, select=None, K=None):
    f = c["f"]
    f.mask_field = c["mfs"][K or c["K0"]]
    res = f.render_objects(t, _cuda(o), _cuda(d), select=select, white_bg=c["white"])
    return [x.cpu().numpy() for x in res]


def _params(c, K=None):
    return o64.mask_params(c["mfs"][K or c["K0"]].state_dict())


def _check(c, res, o, d, t, label, select=None, K=None, floors=None):
    """layers against the yardstick on the device's weights, the maps of a selected render by the map rule; returns the float64 yardstick"""
    mp = _params(c, K)
    y64 = o64.objects64(c["field"], mp, o, d, t, c["white"], select=select, weights=res[3])
    y32 = o64.objects64(c["field"], mp, o, d, t, c["white"], select=select, weights=res[3], dtype=torch.float32)
    R = len(o)
    own = o64.layer_floor(y32, y64)
    got = dict(obj_rgb=res[5], obj_acc=res[6], obj_depth=res[7])
    for i, k in enumerate(o64.LAYER_KEYS):
        floor = floors[i] if floors is not None else own[i]
        err = o64.rel_err(got[k], y64[k])
        print(f"[objects] {label}:{k}: M={y64['M']} max |map| {np.abs(y64[k]).max():.4g}, device {err:.2e}, fp32 yardstick {own[i]:.2e}, bound {4 * floor:.2e}")
        if np.abs(y64[k]).max() == 0:
            assert not got[k].any(), (label, k)
        else:
            assert err <= 4 * floor, (label, k, err, 4 * floor)
    assert np.array_equal(res[6], res[4]), (label, "obj_acc must carry the bits of mask_map")
    zero = ~y64["mask"].any(1)
    for k in o64.LAYER_KEYS:
        assert not got[k][zero].any(), (label, k, "a ray without masked samples must be exactly zero")
    # identity against the device's own pre-background colour: rgb before the white background and the clamp
    pre = res[0].astype(np.float64) - ((1.0 - res[2].astype(np.float64))[:, None] if c["white"] else 0.0)
    inside = (res[0] > 0).all(1) & (res[0] < 1).all(1)          # rays the clamp did not touch
    ident = np.abs(res[5].astype(np.float64).sum(1) - pre)[inside]
    bound = 4 * max(own[0], o64.ulp_floor(y64["obj_rgb"])) * max(np.abs(y64["obj_rgb"]).max(), 1e-30) + 4 * float(np.spacing(np.float32(1.0)))
    print(f"[objects] {label}: identity sum_k obj_rgb = pre-background rgb: {ident.max() if ident.size else 0:.2e} (bound {bound:.2e})")
    assert not ident.size or ident.max() <= bound, (label, ident.max(), bound)
    # the render's own maps
    near = np.union1d(y64["near_rays"], y32["near_rays"])
    bad = o64.map_failures(dict(rgb=res[0], depth=res[1], acc=res[2], weight=res[3]), y64, FP32_FLOOR)
    aside = np.unique(np.concatenate(list(bad.values()))) if bad else np.zeros(0, np.int64)
    print(f"[objects] {label}: rays set aside {len(aside)}/{R} (near-threshold rays {len(near)})")
    assert np.isin(aside, near).all(), (label, bad)
    assert len(aside) <= o64.MAX_ASIDE * R, (label, len(aside))
    return y64


@pytest.mark.parametrize("case", sorted(o64.GOLDEN_FLOOR))
def test_golden_cases(ctx, fx, case):
    c = ctx[case[0]]
    o, d = c["o"][::2], c["d"][::2]
    t, sel = float(fx[case + ":t"]), fx[case + ":select"]
    _check(c, _run(c, o, d, t, select=sel), o, d, t, case, select=sel, floors=o64.GOLDEN_FLOOR[case])


@pytest.mark.parametrize("K", [3, 5, 8])
@pytest.mark.parametrize("R", [1, 3, 65, 130])
def test_shapes(ctx, R, K):
    """R: below one workgroup of four rays, not a multiple of it, more than one workgroup; K: 5 is not a multiple of four"""
    c = ctx["B" if K == 3 else "A"]
    idx = np.arange(R) % len(c["o"])
    idx[-1] = 100        # (the last ray hits the object also when R = 1)
    o, d = c["o"][idx], c["d"][idx]
    _check(c, _run(c, o, d, T_NONKEY, K=K), o, d, T_NONKEY, f"R{R}:K{K}", K=K)
    sel = np.linspace(0.0, 1.0, K).astype(np.float32)
    _check(c, _run(c, o, d, T_NONKEY, select=sel, K=K), o, d, T_NONKEY, f"R{R}:K{K}:select", select=sel, K=K)


@pytest.mark.parametrize("K", K_WIDE)
def test_more_than_eight_classes(ctx, K):
    """field A, one non-keyframe time, R = 130: mask_map / obj_acc, the layers and the select render under the bounds of every other case.  The select
    vectors: a ramp over all classes and, at K = 17 and 32, one that keeps only classes >= 16 - rows j and 16 + j of the logit tile sit in the same
    register of the two half-waves, and a mix-up of the two in k_select_fwd would scale the density by the wrong classes' share"""
    c = ctx["A"]
    R = 130
    idx = np.arange(R) % len(c["o"])
    idx[-1] = 100
    o, d = c["o"][idx], c["d"][idx]
    assert c["mfs"][K].mask_fc.weight.shape == (K, 128)
    y = _check(c, _run(c, o, d, T_NONKEY, K=K), o, d, T_NONKEY, f"R{R}:K{K}", K=K)
    assert y["obj_acc"].shape == (R, K) and (np.abs(y["obj_acc"]).max(0) > 0).all(), "every class carries weight on some ray"
    sels = [np.linspace(0.0, 1.0, K).astype(np.float32)]
    if K > 16:
        sels.append((np.arange(K) >= 16).astype(np.float32))
    for i, sel in enumerate(sels):
        ys = _check(c, _run(c, o, d, T_NONKEY, select=sel, K=K), o, d, T_NONKEY, f"R{R}:K{K}:select{i}", select=sel, K=K)
        if i == 1:      # the yardstick itself tells the two halves apart: keeping rows j instead of 16 + j gives another weight map
            swapped = np.zeros(K, np.float32)
            swapped[:K - 16] = 1.0
            other = o64.objects64(c["field"], _params(c, K), o, d, T_NONKEY, c["white"], select=swapped)
            assert np.abs(other["weight"] - ys["weight"]).max() > 1e-3


def test_rays_that_miss_the_box(ctx):
    c = ctx["A"]
    o, d = c["o"][[3, 100, 200]], -c["d"][[3, 100, 200]]
    for sel in (None, [1.0] * 8):
        res = _run(c, o, d, T_NONKEY, select=sel)
        assert int(c["f"].last_counters[2]) == 0
        assert not any(res[i].any() for i in (4, 5, 6, 7))
        assert not res[2].any()


def test_single_masked_sample(ctx):
    """a bundle in which some ray holds exactly one masked sample: grazing rays towards the edges of the box (the recipe of tests/test_gpu_flow.py)"""
    c = ctx["B"]
    rng = np.random.default_rng(11)
    n = 768
    ab = c["field"].aabb.numpy().astype(np.float64)
    q = rng.uniform(-1, 1, (n, 3))
    ax = rng.integers(0, 3, n)
    q[np.arange(n), ax] = np.sign(q[np.arange(n), ax]) * rng.uniform(0.97, 1.0, n)
    q[np.arange(n), (ax + 1) % 3] = np.sign(q[np.arange(n), (ax + 1) % 3]) * rng.uniform(0.9, 1.03, n)
    dg = (q + 1) / 2 * (ab[1] - ab[0]) + ab[0] - c["o"][0]
    o = np.tile(c["o"][:1], (n, 1)).astype(np.float32)
    d = (dg / np.linalg.norm(dg, axis=1, keepdims=True)).astype(np.float32)
    w = _run(c, o, d, T_NONKEY)[3]
    counts = (w > np.float32(c["field"].thres)).sum(1)
    one = np.nonzero(counts == 1)[0]
    assert len(one), "no ray of the pool holds exactly one masked sample"
    pick = np.concatenate([one[:3], np.nonzero(counts > 1)[0][:6], np.nonzero(counts == 0)[0][:2]])
    o, d = o[pick], d[pick]
    res = _run(c, o, d, T_NONKEY)
    assert ((res[3] > np.float32(c["field"].thres)).sum(1) == 1).any()
    _check(c, res, o, d, T_NONKEY, "one-sample")


def test_repeats_bit_for_bit(ctx):
    c = ctx["A"]
    sel = [1, 1, 0.5, 1, 0, 1, 0.25, 1.0]
    a, b = _run(c, c["o"], c["d"], T_NONKEY, select=sel), _run(c, c["o"], c["d"], T_NONKEY, select=sel)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", "AB")
def test_select_none_is_render_fwd(ctx, kind):
    """select=None: rgb, depth, acc, weights (and the mask map) carry the bits of the plain eval render"""
    c = ctx[kind]
    f = c["f"]
    f.mask_field = c["mfs"][c["K0"]]
    for t in (T_NONKEY, 0.0):
        res = _run(c, c["o"], c["d"], t)
        with torch.no_grad():
            ref = f(t, _cuda(c["o"]), _cuda(c["d"]), white_bg=c["white"])
        for i in range(5):
            assert np.array_equal(res[i], ref[i].cpu().numpy()), (kind, t, i)


@pytest.mark.parametrize("kind", "AB")
def test_select_all_zeros(ctx, kind):
    c = ctx[kind]
    res = _run(c, c["o"], c["d"], T_NONKEY, select=[0.0] * c["K0"])
    assert not res[2].any() and not res[3].any()
    assert np.array_equal(res[0], np.full_like(res[0], 1.0 if c["white"] else 0.0))
    assert not any(res[i].any() for i in (4, 5, 6, 7))


@pytest.mark.parametrize("kind", "AB")
def test_removal_reveals_what_is_behind(ctx, kind):
    c = ctx[kind]
    K = c["K0"]
    full = _run(c, c["o"], c["d"], T_NONKEY)
    dom = int(full[6].sum(0).argmax())
    sel = np.ones(K, np.float32)
    sel[dom] = 0.0
    cut = _run(c, c["o"], c["d"], T_NONKEY, select=sel)
    y64 = _check(c, cut, c["o"], c["d"], T_NONKEY, f"{kind}:removed{dom}", select=sel)
    rest = [k for k in range(K) if k != dom]
    floor = max(o64.GOLDEN_FLOOR[f"{kind}:nr"][1], o64.ulp_floor(y64["obj_acc"]))
    thres = np.float32(c["field"].thres)
    wf, wc = full[3].astype(np.float64), cut[3].astype(np.float64)
    in_full, in_cut = full[3] > thres, cut[3] > thres
    full_rest = full[6][:, rest].sum(1).astype(np.float64)
    s = y64["s"]                                                  # (R, S) float64: s_j = 1 - m_j,dom of the yardstick (1 where no sample is valid)
    # rounding: 4 x the layer floor of the map scale per remaining object, and the map rule's tolerance of an acc-type sum for the device's w'
    fp = 4 * floor * max(float(np.abs(full[6]).max()), 1e-30) * len(rest) + o64.MAP_RTOL * full_rest + FP32_FLOOR["acc"]
    dropped = (in_full & ~in_cut).sum(1)
    soft = np.where(in_full, wf * s * (1.0 - s), 0.0).sum(1)
    bound = fp + dropped * float(thres) + soft
    gain = cut[6][:, rest].sum(1).astype(np.float64) - full_rest
    print(f"[objects] {kind}: removed object {dom}: layer acc of the rest changes by {gain.min():.3e} .. {gain.max():.3e}; softness term up to "
          f"{soft.max():.3e}, slack min {(gain + bound).min():.3e}")
    assert (gain >= -bound).all(), (kind, (gain + bound).min())
    # the sharp form: everything the selected render accumulates on a ray is at least what the remaining objects had in the full render
    sharp = cut[2].astype(np.float64) - full_rest
    print(f"[objects] {kind}: acc of the selected render - layer acc of the rest in the full render: min {sharp.min():.3e}")
    assert (sharp >= -fp).all(), (kind, sharp.min())
    # and something IS revealed: some sample behind the removed object carries visibly more weight than before
    assert (wc - wf).max() > 1e-3, "removing the object in front must reveal something"


def test_renderer_two_chunks(ctx):
    from nvfi_amd.models import Ray, Renderer
    c = ctx["A"]
    c["f"].mask_field = c["mfs"][8]
    rays = Ray(_cuda(c["o"]).reshape(16, 16, 3), _cuda(c["d"]).reshape(16, 16, 3), 0, 1)
    sel = [0, 2, 3, 5]           # integer entries: the objects to keep
    one = Renderer(c["model"], 0, 0, 256).render_objects(T_NONKEY, rays, select=sel, white_background=c["white"])
    ren = Renderer(c["model"], 0, 0, 128)
    ren.eval_chunk = 128
    two = ren.render_objects(T_NONKEY, rays, select=sel, white_background=c["white"])
    assert ren._eval_chunk(T_NONKEY, False, objects=True) == 128
    assert one[5].shape == (16, 16, 8, 3) and one[6].shape == (16, 16, 8) and one[4].shape == (16, 16, 8)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    keep = np.zeros(8, np.float32)
    keep[sel] = 1.0
    ref = c["f"].render_objects(T_NONKEY, _cuda(c["o"]), _cuda(c["d"]), select=keep, white_bg=c["white"])
    assert torch.equal(one[0].reshape(-1, 3), ref[0])


def test_errors(ctx):
    from nvfi_amd import _lib
    c = ctx["A"]
    f = c["f"]
    o, d = _cuda(c["o"][:8]), _cuda(c["d"][:8])
    f.mask_field = c["mfs"][8]
    f.train()
    try:
        with pytest.raises(NotImplementedError):
            f.render_objects(T_NONKEY, o, d)
    finally:
        f.eval()
    with pytest.raises(_lib.NvfiError):
        f.render_objects(T_NONKEY, o.cpu(), d.cpu())
    with pytest.raises(ValueError):
        f.render_objects(T_NONKEY, o, d, select=[1.0, 0.0])
    f.mask_field = None
    with pytest.raises(NotImplementedError):
        f.render_objects(T_NONKEY, o, d)
    # the C calls: a workspace planned without the flags, and NVFI_TRAIN
    f.mask_field = mf = c["mfs"][8]
    L = _lib.lib()
    md = _lib.MaskDesc()
    md.n_layer, md.n_dim, md.mask_dim = 4, 128, 8
    for i, lin in enumerate(list(mf.point_fc) + [mf.mask_fc]):
        md.W[i] = _lib.ptr(lin.weight); md.b[i] = _lib.ptr(lin.bias)
    desc = f._desc()
    R, S = 8, desc.n_samples
    t = float(np.float32(T_NONKEY))
    nb = C.c_int64(0)
    _lib.check(L.nvfi_render_workspace_bytes_t(C.byref(desc), C.c_int64(R), C.c_int(0), C.c_float(t), C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    rgb, depth, acc, w = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, S, device="cuda")
    layers = [torch.zeros(R, 8, 3, device="cuda"), torch.zeros(R, 8, device="cuda"), torch.zeros(R, 8, device="cuda")]
    sel = torch.ones(8, device="cuda")

    def objects(flags):
        return L.nvfi_render_objects(C.byref(desc), C.byref(md), C.c_int64(R), C.c_float(t), C.c_int(flags), _lib.ptr(w), _lib.ptr(layers[0]),
                                     _lib.ptr(layers[1]), _lib.ptr(layers[2]), _lib.ptr(ws), C.c_int64(ws.numel()), None)

    def select(flags):
        return L.nvfi_render_fwd_select(C.byref(desc), C.byref(md), _lib.ptr(sel), C.c_int64(R), _lib.ptr(o), _lib.ptr(d), None, C.c_float(t),
                                        C.c_int(flags), _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(w), _lib.ptr(ws),
                                        C.c_int64(ws.numel()), None, None)

    assert objects(0) == 2                                                   # planned without NVFI_WANT_MASK
    assert objects(_lib.NVFI_WANT_MASK) == 2                                 # the flag alone does not make the workspace larger
    assert objects(_lib.NVFI_WANT_MASK | _lib.NVFI_TRAIN) == 2
    assert select(0) == 2                                                    # planned without NVFI_WANT_SELECT
    assert select(_lib.NVFI_WANT_SELECT | _lib.NVFI_TRAIN) == 2
    assert select(_lib.NVFI_WANT_SELECT) == 4                                # the workspace is too small for the plan of the flag
    torch.cuda.synchronize()
