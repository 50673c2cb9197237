"""The flow branch of an eval-mode render on the device (flow.hip: nvfi_render_flow; TensorVMKeyframeTimeKplane.render_flow, Renderer.render_flow)
against its float64 restatement (tests/flow64.py, pinned to the reference by tests/test_flow_golden.py), fields A and B.  The yardstick is always
fed the DEVICE's own weight map, so a sample's membership of the masked list is the same on both sides.

Bound: per map, max |device - yardstick(float64)| / max |yardstick| <= 4 x the plain-fp32 floor of that case - flow64(float32) against
flow64(float64), measured on the CPU, never the device's output.  For the golden cases the floor is flow64.GOLDEN_FLOOR[case] (measured by
tests/golden/make_golden_flow.py, re-measured by tests/test_flow_golden.py).  For the shape cases it is measured here, on the case's own rays, time, dt and device
weights, and that measurement alone is the floor, with two lower limits against luck, neither taken from the device: (a) one fp32 ulp of the
map's own scale, spacing(float32(max |map|)) / max |map| <= 1.2e-7: no fp32 map is better than its last bit; (b) in the two tests whose cases
go down to a single masked sample (test_ray_counts, test_masked_counts) the golden entry of the SAME field, time and dt - <kind>:c1 for
t = 19/60, dt = +ts/4 and B:c2 for t = 19/60, dt = -1.3 ts (flow64.GOLDEN_FLOOR; B:c2 is 3.2e-7 / 4.1e-7 / 1.6e-6): the error of one sample is
one draw, and the largest of 256 rays at the same dt is what such a draw can reach.  The factor 4
covers the device's summation order (eight partial sums per ray) and the engine's own sin / cos / SiLU (bounded in tests/test_gpu_x6.py).
Edge cap: a ray may be set aside only when the yardstick reports a sample of it within 4 fp32 ulp of a gate or box face; at most 1 ray in 256 and
never more than one per case.
Golden cases additionally follow the project's 1e-4 contract against the REFERENCE's maps (rtol 1e-4 of the map scale + 4 ulp of it; at most
0.5 % of the rays, at least 1, in the threshold-flip band of 1e-4 of the scale, none outside)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import flow64 as f64
import render64 as r64
from conftest import GOLD
from helpers import field_state, make_model, select_rays

pytestmark = pytest.mark.gpu
T_NONKEY = 19.0 / 60.0


@pytest.fixture(scope="module")
def flow_gold():
    return np.load(os.path.join(GOLD, "flow.npz"))


@pytest.fixture(scope="module")
def ctx(gold, flow_gold):
    out = {}
    for kind in "AB":
        model, meta = make_model(kind)
        model.eval()
        f = model.nvfi
        o, d = gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"]
        cam = (flow_gold[f"{kind}:pose"], int(flow_gold[f"{kind}:H"]), int(flow_gold[f"{kind}:W"]), float(flow_gold[f"{kind}:focal"]))
        ts = f.tmax / (f.num_keyframes - 1)
        out[kind] = dict(model=model, f=f, field=r64.Field(*field_state(model)), o=o, d=d, cam=cam, ts=ts, white=bool(meta["white_background"]))
    return out


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(c, o, d, t, dt, cam=True, transfer=False):
    res = c["f"].render_flow(t, _cuda(o), _cuda(d), dt, camera=c["cam"] if cam else None, white_bg=c["white"], transfer_vel=transfer)
    return [None if x is None else x.cpu().numpy() for x in res]


def _check(c, kind, res, o, d, t, dt, label, floors=None, cam=True, same_dt=None):
    """device maps against the float64 yardstick on the device's weights; returns the yardstick.  floors: the golden case's own entry;
    otherwise the floor is measured here, not below one ulp of the map scale nor below the golden case `same_dt` of the same field, t and dt"""
    w = res[3]
    cm = c["cam"] if cam else None
    y64 = f64.flow64(c["field"], o, d, t, dt, w, cm)
    y32 = f64.flow64(c["field"], o, d, t, dt, w, cm, dtype=torch.float32)
    R = len(o)
    edge = np.union1d(y64["edge_rays"], y32["edge_rays"])
    aside = []
    for i, k in enumerate(f64.MAP_KEYS):
        got = res[4 + i]
        if k not in y64:
            assert got is None
            continue
        ref = y64[k]
        own = f64.rel_err(y32[k], ref)
        scale = np.abs(ref).max()
        ulp = float(np.spacing(np.float32(scale))) / scale if scale > 0 else 0.0
        floor = floors[i] if floors is not None else max(own, ulp, f64.GOLDEN_FLOOR[same_dt][i] if same_dt else 0.0)
        err = np.abs(got.astype(np.float64) - ref).max(-1) / scale if scale > 0 else np.abs(got).max(-1)
        print(f"[flow] {label}:{k}: M={y64['M']} max |map| {scale:.4g}, device {err.max() if R else 0:.2e}, fp32 yardstick {own:.2e}, bound {4 * floor:.2e}")
        bad = np.nonzero(err > 4 * floor)[0]
        assert np.isin(bad, edge).all(), (label, k, bad, err[bad], 4 * floor)
        aside = np.union1d(aside, bad)
        if scale == 0:
            assert not got.any(), (label, k)
    assert len(aside) <= min(1, R // 256), (label, "rays set aside", aside)
    zero = ~y64["mask"].any(1)
    for got in res[4:]:
        if got is not None:
            assert not got[zero].any(), (label, "a ray without masked samples must be exactly zero")
    return y64


CASES = sorted(f64.GOLDEN_FLOOR)
_golden_runs = {}


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(ctx, flow_gold, case):
    kind = case[0]
    c = ctx[kind]
    t, dt, transfer = float(flow_gold[case + ":t"]), float(flow_gold[case + ":dt"]), bool(flow_gold[case + ":transfer"])
    res = _run(c, c["o"], c["d"], t, dt, transfer=transfer)
    _golden_runs[case] = res
    _check(c, kind, res, c["o"], c["d"], t, dt, case, floors=f64.GOLDEN_FLOOR[case])
    # the 1e-4 contract against the reference's maps
    R = len(c["o"])
    for i, k in enumerate(f64.MAP_KEYS):
        ref = flow_gold[f"{case}:{k}"].astype(np.float64)
        got = res[4 + i].astype(np.float64)
        scale = np.abs(ref).max()
        if scale == 0:
            assert not got.any()
            continue
        err = np.abs(got - ref).max(-1)
        tol = 1e-4 * scale + 4 * np.spacing(np.float32(scale))
        n_bad = int((err > tol).sum())
        print(f"[flow contract] {case}:{k}: max err / scale {err.max() / scale:.2e}, rays outside: {n_bad}/{R}")
        assert n_bad <= max(1, int(0.005 * R)), (case, k, n_bad)
        assert err.max() <= tol + 1e-4 * scale, (case, k, err.max(), scale)


@pytest.mark.parametrize("kind", "AB")
@pytest.mark.parametrize("R", [1, 3, 5, 257])
def test_ray_counts(ctx, kind, R):
    c = ctx[kind]
    idx = np.arange(R) % len(c["o"])
    idx[-1] = 100        # (the last ray hits the object also when R = 1)
    o, d = c["o"][idx], c["d"][idx]
    dt = c["ts"] / 4
    _check(c, kind, _run(c, o, d, T_NONKEY, dt), o, d, T_NONKEY, dt, f"{kind}:R{R}", same_dt=f"{kind}:c1")


_counts = {}


def _pool(c, kind, n=768):
    """the golden rays behind `n` grazing rays from the same camera position towards points near the edges of the box (short chords: lists of a
    few samples per ray; the recipe of tests/render64_worker.py), with the device's masked count per ray - rendered once"""
    if kind not in _counts:
        rng = np.random.default_rng(11)
        ab = c["field"].aabb.numpy().astype(np.float64)
        q = rng.uniform(-1, 1, (n, 3))
        ax = rng.integers(0, 3, n)
        q[np.arange(n), ax] = np.sign(q[np.arange(n), ax]) * rng.uniform(0.97, 1.0, n)
        q[np.arange(n), (ax + 1) % 3] = np.sign(q[np.arange(n), (ax + 1) % 3]) * rng.uniform(0.9, 1.03, n)
        dg = (q + 1) / 2 * (ab[1] - ab[0]) + ab[0] - c["o"][0]
        o = np.concatenate([np.tile(c["o"][:1], (n, 1)), c["o"]]).astype(np.float32)
        d = np.concatenate([dg / np.linalg.norm(dg, axis=1, keepdims=True), c["d"]]).astype(np.float32)
        w = _run(c, o, d, T_NONKEY, 0.0, cam=False)[3]
        _counts[kind] = (o, d, (w > np.float32(c["field"].thres)).sum(1))
    return _counts[kind]


@pytest.mark.parametrize("M", [0, 1, 31, 32, 33, 127, 128, 129])
def test_masked_counts(ctx, M):
    """the 32-sample tile and 128-sample workgroup edges of the velocity kernels' lists (field B)"""
    c = ctx["B"]
    po, pd, counts = _pool(c, "B")
    if M == 0:
        o, d = c["o"][[3, 100, 200]], -c["d"][[3, 100, 200]]          # rays that point away from the box: nothing valid, nothing masked
    else:
        sel = select_rays(counts, M)
        assert sel is not None, M
        o, d = po[sel], pd[sel]
    dt = -1.3 * c["ts"]
    res = _run(c, o, d, T_NONKEY, dt)
    assert int(c["f"].last_counters[2]) == M
    _check(c, "B", res, o, d, T_NONKEY, dt, f"B:m{M}", same_dt="B:c2")
    if M == 0:
        assert not any(x.any() for x in res[4:])


def test_many_samples(ctx):
    """about 33 k masked samples (field B, the golden rays five times over): more than a thousand 32-sample tiles"""
    c = ctx["B"]
    o, d = np.tile(c["o"], (5, 1)), np.tile(c["d"], (5, 1))
    dt = c["ts"] / 4
    res = _run(c, o, d, T_NONKEY, dt)
    M = int(c["f"].last_counters[2])
    assert 30000 < M < 40000, M
    _check(c, "B", res, o, d, T_NONKEY, dt, "B:many")
    for x in res[4:]:
        assert np.array_equal(x[:256], x[256:512]) and np.array_equal(x[:256], x[1024:])


@pytest.mark.parametrize("kind", "AB")
@pytest.mark.parametrize("key", [False, True])
@pytest.mark.parametrize("dtk", ["zero", "quarter", "back", "beyond"])
def test_times(ctx, kind, key, dtk):
    c = ctx[kind]
    t = 2 * c["ts"] if key else T_NONKEY
    dt = dict(zero=0.0, quarter=c["ts"] / 4, back=-1.3 * c["ts"], beyond=c["f"].tmax - t + 0.07)[dtk]
    o, d = c["o"][64:192], c["d"][64:192]
    res = _run(c, o, d, t, dt)
    _check(c, kind, res, o, d, t, dt, f"{kind}:{'key' if key else 'nonkey'}:{dtk}")
    if dtk == "zero":
        assert not res[5].any() and not res[6].any() and res[4].any()


@pytest.mark.parametrize("kind", "AB")
def test_transfer_and_no_camera(ctx, kind):
    c = ctx[kind]
    o, d, dt = c["o"][64:192], c["d"][64:192], c["ts"] / 4
    res = _run(c, o, d, T_NONKEY, dt, transfer=True)
    _check(c, kind, res, o, d, T_NONKEY, dt, f"{kind}:transfer")
    res2 = _run(c, o, d, T_NONKEY, dt, cam=False, transfer=True)
    assert res2[6] is None
    for a, b in zip(res[:6], res2[:6]):
        assert np.array_equal(a, b)


def _raw(f, o, d, t, dt, plan_flags, call_flags, pose=None, cam=(0, 0, 0.0), outs=(True, True, True), desc_edit=None, edit_first=False):
    """nvfi_render_fwd + nvfi_render_flow through the C ABI; returns rc of the flow call and the three maps (NaN-filled where not asked for)"""
    from nvfi_amd import _lib
    from nvfi_amd.models.tensorf_keyframe import _stream_ptr
    L = _lib.lib()
    o, d = _cuda(o), _cuda(d)
    R = o.shape[0]
    desc = f._desc()
    if desc_edit and edit_first:         # (otherwise the edit reaches the flow call alone)
        desc_edit(desc)
    nb = C.c_int64(0)
    _lib.check(L.nvfi_render_workspace_bytes_t(C.byref(desc), C.c_int64(R), C.c_int(plan_flags), C.c_float(t), C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    rgb, depth, acc = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    w = torch.empty(R, desc.n_samples, device="cuda")
    _lib.check(L.nvfi_render_fwd(C.byref(desc), C.c_int64(R), _lib.ptr(o), _lib.ptr(d), None, C.c_float(t), C.c_int(plan_flags & ~1), _lib.ptr(rgb),
                                 _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(w), _lib.ptr(ws), C.c_int64(ws.numel()), None, _stream_ptr()))
    maps = [torch.full((R, n), float("nan"), device="cuda") for n in (3, 3, 2)]
    if desc_edit and not edit_first:
        desc_edit(desc)
    rc = L.nvfi_render_flow(C.byref(desc), C.c_int64(R), _lib.ptr(o), _lib.ptr(d), C.c_float(t), C.c_float(dt), C.c_int(call_flags), _lib.ptr(w),
                            _lib.ptr(pose), C.c_int(cam[0]), C.c_int(cam[1]), C.c_float(cam[2]),
                            *[_lib.ptr(m) if on else None for m, on in zip(maps, outs)], _lib.ptr(ws), C.c_int64(ws.numel()), _stream_ptr())
    torch.cuda.synchronize()
    return rc, [m.cpu().numpy() for m in maps]


def test_optional_outputs_and_errors(ctx):
    from nvfi_amd import _lib
    c = ctx["A"]
    f, o, d, dt = c["f"], c["o"][96:160], c["d"][96:160], c["ts"] / 4
    FL = _lib.NVFI_WANT_FLOW
    pose = _cuda(c["cam"][0])
    cam = (c["cam"][1], c["cam"][2], c["cam"][3])
    rc, full = _raw(f, o, d, T_NONKEY, dt, FL, FL, pose, cam)
    assert rc == 0 and all(np.isfinite(m).all() for m in full)
    for skip in range(3):         # each output pointer NULL in turn: the others are the full call's, bit for bit; the skipped one is not touched
        outs = tuple(i != skip for i in range(3))
        rc, part = _raw(f, o, d, T_NONKEY, dt, FL, FL, pose, cam, outs)
        assert rc == 0
        for i in range(3):
            assert np.isnan(part[i]).all() if i == skip else np.array_equal(part[i], full[i]), (skip, i)
    rc, nop = _raw(f, o, d, T_NONKEY, dt, FL, FL, None)            # no pose: flow2d is skipped
    assert rc == 0 and np.isnan(nop[2]).all() and np.array_equal(nop[0], full[0]) and np.array_equal(nop[1], full[1])
    assert _raw(f, o, d, T_NONKEY, dt, 0, 0, pose, cam)[0] == 2                       # workspace planned without NVFI_WANT_FLOW
    assert _raw(f, o, d, T_NONKEY, dt, FL, 0, pose, cam)[0] == 2
    assert _raw(f, o, d, T_NONKEY, dt, FL, FL | _lib.NVFI_TRAIN, pose, cam)[0] == 2   # a train-mode call
    assert _raw(f, o, d, T_NONKEY, dt, FL, FL, pose, cam, desc_edit=lambda ds: setattr(ds, "use_vel", 0))[0] == 2
    assert _raw(f, o, d, T_NONKEY, 65 * 0.5 * c["ts"], FL, FL, pose, cam)[0] == 2     # more RK2 steps than the library's limit: refused
    assert b"RK2 steps" in _lib.lib().nvfi_last_error()
    assert _raw(f, o, d, T_NONKEY, dt, 0, FL, pose, cam)[0] == 2                      # ... whatever the flow call's own flags say
    with pytest.raises(_lib.NvfiError):
        f.render_flow(T_NONKEY, torch.from_numpy(o), torch.from_numpy(d), dt)
    f.train()
    try:
        with pytest.raises(NotImplementedError):
            f.render_flow(T_NONKEY, _cuda(o), _cuda(d), dt)
    finally:
        f.eval()
    m0, _ = make_model("A", use_vel=False)
    m0.eval()
    with pytest.raises(NotImplementedError):
        m0.nvfi.render_flow(T_NONKEY, _cuda(o), _cuda(d), dt)


@pytest.mark.parametrize("key", [False, True])
def test_descriptor_without_fragment_cache(ctx, key):
    """what a plain C caller gets: a descriptor with frags = NULL, so both calls pack the velocity net's fragments and its x6 image into the
    workspace (flow.hip: launch_pack into vel_frag, launch_pack_x6 into the branch's own image; a keyframe render plans no x6 image of its
    own).  The same weights through the same pack kernels: the maps are those of the cached descriptor bit for bit"""
    from nvfi_amd import _lib
    c = ctx["B"]
    f, o, d, dt = c["f"], c["o"][64:192], c["d"][64:192], -1.3 * c["ts"]
    t = 2 * c["ts"] if key else T_NONKEY
    FL = _lib.NVFI_WANT_FLOW
    pose, cam = _cuda(c["cam"][0]), (c["cam"][1], c["cam"][2], c["cam"][3])
    rc, cached = _raw(f, o, d, t, dt, FL, FL, pose, cam)
    assert rc == 0 and f._desc().frags, "the field's own descriptor carries the cache"
    rc, plain = _raw(f, o, d, t, dt, FL, FL, pose, cam, desc_edit=lambda ds: setattr(ds, "frags", None), edit_first=True)
    assert rc == 0
    for a, b in zip(cached, plain):
        assert np.isfinite(b).all() and np.abs(b).max() > 0 and np.array_equal(a, b)


@pytest.mark.parametrize("kind", "AB")
def test_properties(ctx, kind):
    from nvfi_amd.models import Ray, Renderer
    c = ctx[kind]
    o, d, dt = c["o"], c["d"], -1.3 * c["ts"]
    a = _run(c, o, d, T_NONKEY, dt)
    b = _run(c, o, d, T_NONKEY, dt)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                      # two calls are bit-identical
    p = _run(c, o[:77], d[:77], T_NONKEY, dt)
    for x, y in zip(a, p):
        assert np.array_equal(x[:77], y)                 # a prefix of the rays gives the prefix of the maps
    ren = Renderer(c["model"], 0, 0, 2048)
    five = ren.render(T_NONKEY, Ray(_cuda(o), _cuda(d), 0, 1), white_background=c["white"], mode="test")
    for x, y in zip(a[:4], five[:4]):
        assert np.array_equal(x, y.cpu().numpy())        # the ordinary outputs are Renderer.render's
    f = c["f"]
    old = f.vel_fp16
    f.vel_fp16 = "fp32"                                  # descriptor bit 3: the fp32 MFMA integrator (A/B reference)
    try:
        r8 = _run(c, o, d, T_NONKEY, dt)
    finally:
        f.vel_fp16 = old
    _check(c, kind, r8, o, d, T_NONKEY, dt, f"{kind}:fp32-integrator")


def test_renderer_chunks_and_png(ctx, tmp_path):
    """a 200 x 200 frame in five chunks of 8192 rays over both side streams equals the single-chunk frame bit for bit; flow_to_rgb and the
    with_flow PNG of render_test_evaluation go through one small frame"""
    from nvfi_amd.models import Camera, Renderer
    from nvfi_amd.utils import render_test_evaluation
    from nvfi_amd.utils.flow_vis import flow_to_rgb
    c = ctx["A"]
    pose = torch.eye(4)
    pose[:3, :4] = torch.from_numpy(np.asarray(c["cam"][0]))
    H = W = 200
    focal = c["cam"][3] / 4
    cam = Camera(pose.cuda(), H, W, focal, None, 1.0, 8.0)
    ren = Renderer(c["model"], 0, 0, 2048)
    dt = c["ts"] / 4
    ren.eval_chunk = 1 << 20
    one = ren.render_flow(T_NONKEY, cam.rays.to("cuda"), dt, camera=cam, white_background=c["white"])
    ren.eval_chunk = 8192
    five = ren.render_flow(T_NONKEY, cam.rays.to("cuda"), dt, camera=cam, white_background=c["white"])
    assert one[4].shape == (H, W, 3) and one[5].shape == (H, W, 3) and one[6].shape == (H, W, 2)
    for x, y in zip(one, five):
        assert torch.equal(x, y)
    assert float(one[6].abs().max()) > 0.1
    rgb = flow_to_rgb(one[6])
    assert rgb.shape == (H, W, 3) and float(rgb.min()) >= 0 and float(rgb.max()) <= 1 and rgb.is_cuda
    none = ren.render_flow(T_NONKEY, cam.rays.to("cuda"), dt, white_background=c["white"])
    assert none[6] is None and torch.equal(none[5], one[5])
    base = render_test_evaluation(c["model"], ren, [pose], [T_NONKEY], None, 48, 48, focal * 48 / 200, 1.0, 8.0, white_background=c["white"],
                                  savedir=str(tmp_path / "plain"), update_alpha_mask=False)
    flow = render_test_evaluation(c["model"], ren, [pose], [T_NONKEY], None, 48, 48, focal * 48 / 200, 1.0, 8.0, white_background=c["white"],
                                  savedir=str(tmp_path / "flow"), update_alpha_mask=False, with_flow=dt)
    assert np.array_equal(base["images"], flow["images"]) and "flow2d" not in base and flow["flow2d"].shape == (1, 48, 48, 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["r_000.png"]
    assert sorted(os.listdir(tmp_path / "flow")) == ["r_000.png", "r_000_flow.png"]
    assert (tmp_path / "plain" / "r_000.png").read_bytes() == (tmp_path / "flow" / "r_000.png").read_bytes()
    from PIL import Image
    assert Image.open(tmp_path / "flow" / "r_000_flow.png").size == (48, 48)
