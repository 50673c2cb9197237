"""Differentiable field lookups on the device - nvfi_density_grad, nvfi_appfeat_at, nvfi_appfeat_grad (csrc/lookup.hip), their raw wrappers
(nvfi_amd/utils/field_lookup.py) and field.lookup_density / lookup_appfeature / compute_appfeature - against the float64 yardstick tests/lookup64.py,
which tests/test_lookup_golden.py pins to the reference's goldens.  The yardsticks run in torch on the GPU.

Fields: A (K = 4), B (K = 16), D (A's geometry with SH shading: app_dim 27).  Bound of every comparison, the same for every tensor (value, g_xyzt
- all four columns -, each plane gradient, basis_mat's): |got - ref64| <= max(3 x floor, 1e-5 x max |ref64|), floor = the yardstick's float32
evaluation against its float64 evaluation on that case (lookup64.bound; the rule of test_gpu_advect.py / test_gpu_flowloss.py).  Every check
prints `[lookup] <case>: <tensor>: error / bound`.  The contention case (1024 points inside one 2 x 2 x 2 texel cluster, every atomic of the call
on the same texels) holds the same rule: the order-dependent fp32 sums stay at 0.10 .. 0.25 of it, so it is not widened.

Measured on an MI355X, worst error / bound over all cases (test_print_worst prints them): value 0.03 (density; bit-identical to
compute_densityfeature) / 0.33 (appearance), g_xyzt 0.21 / 0.29, plane gradients and basis_mat 0.26 / 0.26; chained behind advect, x.grad 0.10 and
the twelve weight_net gradients 0.09 - 0.13.  The file takes 6 s; no test over 1.2 s."""
import os

import numpy as np
import pytest
import torch

import advect64 as a64
import lookup64 as l64
import point64 as p64
from conftest import GOLD
from helpers import field_state, make_model

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
KINDS = ("A", "B", "D")
SENT = -7.0
WORST = {}


@pytest.fixture(scope="module")
def dev():
    """fields A, B and D: the device field and the yardstick's field of the same parameters"""
    from test_gpu_charloss import sh_model
    out = {}
    for kind in KINDS:
        model = sh_model() if kind == "D" else make_model(kind)[0]
        model.eval()
        out[kind] = (model.nvfi, p64.field_of(*field_state(model), sh=kind == "D"))
    return out


def _fl():
    from nvfi_amd.utils import field_lookup
    return field_lookup


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _geom(f):
    return [int(v) for v in f.gridSize.tolist()], int(f.num_keyframes)


def _params(f, family):
    return f._render_params()[:6] if family == "density" else f._render_params()[6:13]


def _names(family):
    return l64.D_NAMES if family == "density" else l64.A_NAMES


def _inputs(f, family, N, seed, q=None):
    rng = np.random.default_rng(seed)
    grid, K = _geom(f)
    if q is None:
        q = l64.point_mix(rng, N, grid, K)
    g = rng.standard_normal((len(q),) if family == "density" else (len(q), int(f.app_dim))).astype(np.float32)
    return q, g


_yard = {}


def _yardstick(dev, kind, family, q, g, key=None):
    """(float64, float32) yardstick tensors of a case (lookup64.tensors), computed once per key"""
    if key is not None and (kind, family, key) in _yard:
        return _yard[(kind, family, key)]
    fn = l64.density_lookup64 if family == "density" else l64.app_lookup64
    y = (l64.tensors(fn(dev[kind][1], q, g, device="cuda")), l64.tensors(fn(dev[kind][1], q, g, dtype=torch.float32, device="cuda")))
    if key is not None:
        _yard[(kind, family, key)] = y
    return y


def _buffers(f, family, which=None, fill=0.0):
    """gradient buffers in the parameters' own layout (None where not asked for) and the nvfi_grads that points at them"""
    names, params = _names(family), _params(f, family)
    bufs = [torch.full_like(p, fill) if (which is None or n in which) else None for n, p in zip(names, params)]
    return bufs, f._grads_struct(bufs if family == "density" else [None] * 6 + bufs)


def _raw(f, family, q, g, want_q=True, which=None, bufs=None, gq=None):
    """one raw backward call -> {label: numpy} in lookup64.tensors' labels (without `value`), and the device tensors"""
    fl = _fl()
    if bufs is None:
        bufs, G = _buffers(f, family, which)
    else:
        G = f._grads_struct(bufs if family == "density" else [None] * 6 + bufs)
    call = fl.density_grad_raw if family == "density" else fl.appfeat_grad_raw
    out = call(f._desc(), _cu(q), _cu(g), g_xyzt=(gq if gq is not None else True) if want_q else None, grads=G)
    torch.cuda.synchronize()
    got = {} if out is None else {"g_xyzt": out.cpu().numpy()}
    for n, b in zip(_names(family), bufs):
        if b is not None:
            got["grad:" + n] = b.cpu().numpy()
    return got, out, bufs


def _check(label, got, t64, t32, scale=1.0):
    """every tensor of `got` (divided by `scale`) inside the bound of its yardstick entry; prints error / bound"""
    for k, v in got.items():
        ref = t64[k]
        b = l64.bound(ref, t32[k])
        err = np.abs(np.asarray(v, np.float64) / scale - ref)
        assert err.shape == ref.shape, (label, k, err.shape, ref.shape)
        e = float(err.max()) if err.size else 0.0
        ratio = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        print(f"[lookup] {label}: {k}: max |ref64| {np.abs(ref).max() if ref.size else 0:.3g}, error {e:.2e}, float32 floor {l64.max_err(t32[k], ref):.2e}, "
              f"bound {b:.2e}, error / bound {ratio:.2f}", flush=True)
        WORST[k.split(":")[0] + ":" + label.split(":")[1]] = max(WORST.get(k.split(":")[0] + ":" + label.split(":")[1], 0.0), ratio)
        assert e <= b, (label, k, e, b, ratio)


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("kind", KINDS)
def test_values(dev, gold, kind):
    f = dev[kind][0]
    q, g = _inputs(f, "app", 257, 5)
    qt = _cu(q)
    d0 = f.compute_densityfeature(qt)
    assert torch.equal(f.lookup_density(qt), d0) and d0.shape == (257, 1)
    with torch.no_grad():
        assert torch.equal(f.lookup_density(qt.clone().requires_grad_(True)), d0)
    d1 = f.lookup_density(qt.clone().requires_grad_(True))
    assert d1.requires_grad and torch.equal(d1.detach(), d0), "lookup_density's value is compute_densityfeature's bit for bit"
    feat = _fl().appfeat_raw(f._desc(), qt)
    assert feat.shape == (257, int(f.app_dim)) and int(f.app_dim) == (27 if kind == "D" else 32)
    assert torch.equal(f.compute_appfeature(qt), feat) and not f.compute_appfeature(qt.clone().requires_grad_(True)).requires_grad
    a1 = f.lookup_appfeature(qt.clone().requires_grad_(True))
    assert a1.requires_grad and torch.equal(a1.detach(), feat)
    t64, t32 = _yardstick(dev, kind, "app", q, g, key="values")
    _check(f"{kind}:app:values", {"value": feat.cpu().numpy()}, t64, t32)
    t64d, t32d = _yardstick(dev, kind, "density", q, g[:, 0], key="values")
    _check(f"{kind}:density:values", {"value": d0[:, 0].cpu().numpy()}, t64d, t32d)
    if kind != "D":
        # the reference's own fp32 features (hotpath.npz): device and golden each sit within the bound of the yardstick
        xyzt = gold[f"{kind}:feat:xyzt"]
        got = f.compute_appfeature(_cu(xyzt)).cpu().numpy()
        y64 = l64.app_lookup64(dev[kind][1], xyzt, device="cuda")["value"]
        y32 = l64.app_lookup64(dev[kind][1], xyzt, dtype=torch.float32, device="cuda")["value"]
        b = l64.bound(y64, y32)
        e, eg = l64.max_err(got, y64), l64.max_err(got, gold[f"{kind}:feat:app"])
        print(f"[lookup] {kind}:app:hotpath: value: error {e:.2e} (against the reference's fp32 {eg:.2e}), bound {b:.2e}, error / bound {e / b:.2f}")
        assert e <= b and eg <= 2 * b


# ---------------------------------------------------------------------------------------------------------------- 2. gradients
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_gradients(dev, kind, N):
    f = dev[kind][0]
    for family in ("density", "app"):
        q, g = _inputs(f, family, N, 100 + N)
        t64, t32 = _yardstick(dev, kind, family, q, g, key=N)
        got, _, _ = _raw(f, family, q, g)
        assert set(got) == set(t64) - {"value"}
        _check(f"{kind}:{family}:N={N}", got, t64, t32)


def test_golden_points(dev):
    """the golden points themselves (texel nodes, faces, out-of-range rows) and the reference's fp32 gradients next to the device's"""
    lg = np.load(os.path.join(GOLD, "lookup.npz"))
    for kind in ("A", "B"):
        f = dev[kind][0]
        for family in ("density", "app"):
            q, g = lg[f"{kind}:xyzt"], lg[f"{kind}:{family}:g"]
            t64, t32 = _yardstick(dev, kind, family, q, g, key="golden")
            got, _, _ = _raw(f, family, q, g)
            _check(f"{kind}:{family}:golden", got, t64, t32)
            for k, v in got.items():
                ref = lg[f"{kind}:{family}:{k}"]
                assert l64.max_err(v, ref) <= 2 * l64.bound(t64[k], t32[k]), (kind, family, k)


@pytest.mark.parametrize("family", ("density", "app"))
def test_partial_sets_and_accumulation(dev, family):
    f = dev["A"][0]
    q, g = _inputs(f, family, 65, 165)
    t64, t32 = _yardstick(dev, "A", family, q, g, key=65)
    names = _names(family)
    time_planes = [n for n in names if "_time." in n]
    sets = [("no g_xyzt", False, None), ("time planes", True, time_planes), ("g_xyzt alone", True, [])]
    if family == "app":
        sets.append(("basis alone", False, ["basis_mat.weight"]))
    for label, want_q, which in sets:
        got, _, _ = _raw(f, family, q, g, want_q=want_q, which=which)
        assert set(got) == ({"g_xyzt"} if want_q else set()) | {"grad:" + n for n in (names if which is None else which)}, label
        _check(f"A:{family}:{label}", got, t64, t32)
    # buffers that hold values are accumulated into: a second call on the same buffers doubles them; g_xyzt is overwritten
    first, gq1, bufs = _raw(f, family, q, g)
    gq = torch.full((65, 4), SENT, device="cuda")
    second, gq2, _ = _raw(f, family, q, g, bufs=bufs, gq=gq)
    assert gq2 is gq and torch.equal(gq1, gq2), "g_xyzt is overwritten, and repeats bit for bit"
    del second["g_xyzt"]
    _check(f"A:{family}:two calls", second, t64, t32, scale=2.0)
    for k in second:
        assert np.abs(second[k]).max() > 1.5 * np.abs(first[k]).max()


# ---------------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("kind", ("A", "D"))
def test_dead_points_give_exact_zeros(dev, kind):
    """every tap of every plane out of range (points beyond the box by more than a texel), and non-finite / far coordinates: value, g_xyzt and
    every gradient buffer are exactly zero, and nothing faults"""
    f = dev[kind][0]
    rng = np.random.default_rng(3)
    outside = np.concatenate([(1.5 + rng.random((40, 3))) * rng.choice([-1.0, 1.0], (40, 3)), rng.random((40, 1)) * 2 - 1], 1).astype(np.float32)
    nan, inf = np.nan, np.inf
    wild = np.array([[nan, 0, 0, 0], [0, nan, 0, 0], [0, 0, nan, 0], [0.1, 0.2, 0.3, nan], [inf, 0, 0, 0], [0, -inf, 0, 0], [0.1, 0.2, 0.3, inf],
                     [0.1, 0.2, 0.3, -inf], [1e6, 0, 0, 0], [0, -1e6, 0.5, 0], [0.1, 0.2, 1e6, 0], [0.1, 0.2, 0.3, 1e6], [3e38, -3e38, 3e38, 3e38],
                     [nan, nan, nan, nan], [0.1, 0.2, 0.3, 50.0], [0.1, 0.2, 0.3, -50.0]], np.float32)
    for label, q in (("outside", outside), ("wild", wild)):
        qt = _cu(q)
        assert not f.compute_appfeature(qt).any(), label
        # (the density VALUE is nvfi_density_at's, which this feature leaves alone: exact zeros at far points - test_gpu_point64.py pins |coordinate|
        # to 1e6 -, its own answer where the fp32 texel coordinate is not finite)
        assert not f.lookup_density(qt[(qt.abs() <= 1e6).all(1)]).any(), label
        for family in ("density", "app"):
            g = np.ones((len(q),) if family == "density" else (len(q), int(f.app_dim)), np.float32)
            got, _, _ = _raw(f, family, q, g, gq=torch.full((len(q), 4), SENT, device="cuda"))
            assert all(not v.any() for v in got.values()), (label, family, [k for k, v in got.items() if v.any()])
    # mixed with live points: the dead ones leave the others' results alone
    live, g = _inputs(f, "density", 33, 9)
    mix = np.concatenate([wild[:8], live, outside[:7]])
    gm = np.concatenate([np.ones(8, np.float32), g, np.ones(7, np.float32)])
    t64, t32 = _yardstick(dev, kind, "density", live, g)
    got, _, _ = _raw(f, "density", mix, gm)
    assert not got["g_xyzt"][:8].any() and not got["g_xyzt"][41:].any()
    got["g_xyzt"] = got["g_xyzt"][8:41]
    _check(f"{kind}:density:mixed with dead points", got, t64, t32)


def test_empty_call(dev):
    f = dev["A"][0]
    fl = _fl()
    q = torch.empty(0, 4, device="cuda")
    assert f.lookup_density(q).shape == (0, 1) and f.compute_appfeature(q).shape == (0, 32)
    for family in ("density", "app"):
        bufs, G = _buffers(f, family, fill=SENT)
        g = torch.empty((0,) if family == "density" else (0, 32), device="cuda")
        out = (fl.density_grad_raw if family == "density" else fl.appfeat_grad_raw)(f._desc(), q, g, grads=G)
        torch.cuda.synchronize()
        assert out.shape == (0, 4) and all(bool((b == SENT).all()) for b in bufs)
    x = q.clone().requires_grad_(True)
    gx, = torch.autograd.grad(f.lookup_density(x).sum() + f.lookup_appfeature(x).sum(), x)
    assert gx.shape == (0, 4)


@pytest.mark.parametrize("kind", ("A", "B"))
def test_time_row_extremes(dev, kind):
    """t' on the first and last row, one fp32 step inside and outside of them, on every row, and a texel beyond either end"""
    f = dev[kind][0]
    grid, K = _geom(f)
    rows = (2.0 * np.arange(K) / (K - 1) - 1.0).astype(np.float32)
    one = np.float32(1)
    tn = np.concatenate([rows, [np.nextafter(-one, -2 * one), np.nextafter(-one, one), np.nextafter(one, 2 * one), np.nextafter(one, -one),
                                -1 - 1.0 / (K - 1), 1 + 1.0 / (K - 1), -1 - 2.5 / (K - 1), 1 + 2.5 / (K - 1)]]).astype(np.float32)
    q = l64.point_mix(np.random.default_rng(17), len(tn), grid, K, extent=0.95, n_nodes=0)
    q[:, 3] = tn
    for family in ("density", "app"):
        _, g = _inputs(f, family, len(q), 18, q=q)
        t64, t32 = _yardstick(dev, kind, family, q, g)
        got, _, _ = _raw(f, family, q, g)
        assert np.abs(t64["g_xyzt"][:, 3]).max() > 0
        assert not got["g_xyzt"][-2:].any() and not t64["g_xyzt"][-2:].any(), "more than a row beyond the planes: nothing is in range"
        _check(f"{kind}:{family}:time rows", got, t64, t32)


# ---------------------------------------------------------------------------------------------------------------- 4. contention
@pytest.mark.parametrize("family", ("density", "app"))
def test_contention(dev, family):
    """1024 points inside one 2 x 2 x 2 texel cluster (and one time-row interval): every atomic of the call lands on the same 8 + 4 texel rows"""
    f, yf = dev["B"]
    grid, K = _geom(f)
    rng = np.random.default_rng(23)
    n = 1024
    cell = [5, 7, 9, 6]
    u = 0.02 + 0.96 * rng.random((n, 4))
    q = np.stack([2.0 * (cell[c] + u[:, c]) / (W - 1) - 1.0 for c, W in enumerate(grid + [K])], 1).astype(np.float32)
    _, g = _inputs(f, family, n, 24, q=q)
    t64, t32 = _yardstick(dev, "B", family, q, g)
    got, _, _ = _raw(f, family, q, g)
    for k in got:
        if k != "g_xyzt":
            assert int((got[k] != 0).sum()) == int((t64[k] != 0).sum()) == (1536 if "basis" in k else 4 * (24 if family == "density" else 48)), k
    _check(f"B:{family}:contention", got, t64, t32)


# ---------------------------------------------------------------------------------------------------------------- 5. repeats
def test_repeats_and_graph_replay(dev):
    """N = 20 011 (the waves grid-stride): two calls and one hipGraph replay give feat and g_xyzt bit for bit; the parameter gradients, float
    atomics, stay within the bound of the yardstick each time"""
    f = dev["A"][0]
    fl = _fl()
    N = 20011
    desc = f._desc()
    for family in ("density", "app"):
        q, g = _inputs(f, family, N, 31)
        t64, t32 = _yardstick(dev, "A", family, q, g)
        qt, gt = _cu(q), _cu(g)
        call = fl.density_grad_raw if family == "density" else fl.appfeat_grad_raw
        runs = []
        for rep in range(2):
            got, gq, _ = _raw(f, family, q, g)
            _check(f"A:{family}:N={N} call {rep}", got, t64, t32)
            runs.append((gq, fl.appfeat_raw(desc, qt) if family == "app" else None))
        assert torch.equal(runs[0][0], runs[1][0])
        bufs, G = _buffers(f, family)
        gq = torch.full((N, 4), SENT, device="cuda")
        feat = torch.full((N, int(f.app_dim)), SENT, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=cap):
            call(desc, qt, gt, g_xyzt=gq, grads=G)
            if family == "app":
                fl.appfeat_raw(desc, qt, out=feat)
        torch.cuda.current_stream().wait_stream(cap)
        for b in bufs:
            b.zero_()
        gq.fill_(SENT)
        feat.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gq, runs[0][0]), (family, "g_xyzt of the replay")
        if family == "app":
            assert torch.equal(feat, runs[0][1]) and torch.equal(runs[0][1], runs[1][1])
            _check(f"A:app:N={N} value", {"value": feat.cpu().numpy()}, t64, t32)
        got = {"grad:" + n: b.cpu().numpy() for n, b in zip(_names(family), bufs)}
        _check(f"A:{family}:N={N} replay", got, t64, t32)


# ---------------------------------------------------------------------------------------------------------------- 6. chain with advect
def test_chain_with_advect(dev):
    """q = cat(advect(x, t, t_k), t'_k) -> lookup_density, lookup_appfeature -> a weighted sum -> backward: x.grad and the twelve weight_net
    gradients are, bit for bit, advect's backward fed the raw calls' g_xyzt[:, :3] by hand; the plane gradients are the raw calls' within the
    bound; and against float64 - lookup64 for the gradient at the advected points, advect64 for the adjoint - under the same rule"""
    f, yf = dev["A"]
    fl = _fl()
    N = 129
    ts = f.tmax / (f.num_keyframes - 1)
    t, tk = 19.0 / 60.0, float(np.float32(ts))
    tnk = float(f.normalize_time_coord(torch.tensor([tk]))[0])
    x, _ = a64.case_inputs(N)
    rng = np.random.default_rng(41)
    gd, ga = rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, 32)).astype(np.float32)
    wparams = f._render_params()[19:31]
    planes = f._render_params()[:13]
    xt = _cu(x).requires_grad_(True)
    col = torch.full((N, 1), tnk, device="cuda")
    qx = torch.cat([f.advect(xt, t, tk), col], 1)
    loss = (f.lookup_density(qx)[:, 0] * _cu(gd)).sum() + (f.lookup_appfeature(qx) * _cu(ga)).sum()
    grads = torch.autograd.grad(loss, [xt] + list(wparams) + list(planes))
    gx, gnet, gpl = grads[0], grads[1:13], grads[13:]
    # by hand
    x2 = _cu(x).requires_grad_(True)
    xk = f.advect(x2, t, tk)
    q = torch.cat([xk.detach(), col], 1)
    assert torch.equal(q, qx.detach())
    rd, gqd, _ = _raw(f, "density", q.cpu().numpy(), gd)
    ra, gqa, _ = _raw(f, "app", q.cpu().numpy(), ga)
    hand = torch.autograd.grad(xk, [x2] + list(wparams), grad_outputs=(gqd + gqa)[:, :3].contiguous())
    assert torch.equal(gx, hand[0]), "x.grad is advect's backward of g_xyzt[:, :3]"
    assert all(torch.equal(a, b) for a, b in zip(gnet, hand[1:])), "the weight_net gradients are advect's backward of g_xyzt[:, :3]"
    assert float(gx.abs().max()) > 0 and all(float(g.abs().max()) > 0 for g in gnet)
    qn = q.cpu().numpy()
    for family, raw, up, sl in (("density", rd, gd, gpl[:6]), ("app", ra, ga, gpl[6:])):
        t64, t32 = _yardstick(dev, "A", family, qn, up)
        _check(f"A:{family}:chain", {"grad:" + n: g.cpu().numpy() for n, g in zip(_names(family), sl)}, t64, t32)
        for n, g in zip(_names(family), sl):
            assert l64.max_err(g.cpu().numpy(), raw["grad:" + n]) <= l64.bound(t64["grad:" + n], t32["grad:" + n]), n
    # against float64: the gradient at the advected points from lookup64, its adjoint from advect64; float32 floor: the same chain in float32
    ref = {}
    for dtype in (torch.float64, torch.float32):
        g3 = (l64.density_lookup64(yf, qn, gd, dtype=dtype, device="cuda")["g_xyzt"] + l64.app_lookup64(yf, qn, ga, dtype=dtype, device="cuda")["g_xyzt"])[:, :3]
        ref[dtype] = a64.advect64(yf, x, t, tk, g3, dtype=dtype, device="cuda")
    got = {"gx": gx.cpu().numpy()}
    got.update({k: g.cpu().numpy() for k, g in zip(a64.NET_NAMES, gnet)})
    _check("A:chain:advect adjoint", got, ref[torch.float64], ref[torch.float32])


# ---------------------------------------------------------------------------------------------------------------- 7. autograd surface
def test_autograd_surface(dev, monkeypatch):
    from nvfi_amd import _lib
    f = dev["A"][0]
    fl = _fl()
    q, _ = _inputs(f, "density", 64, 51)
    seen = []

    def spy(name):
        real = getattr(fl, name)

        def wrapped(desc, xyzt, g, g_xyzt=True, grads=None):
            ptrs = None if grads is None else [bool(p) for arr in (grads.dps, grads.dpt, grads.aps, grads.apt) for p in arr] + [bool(grads.basis)]
            seen.append((name, g_xyzt is not None, ptrs))
            return real(desc, xyzt, g, g_xyzt=g_xyzt, grads=grads)
        monkeypatch.setattr(fl, name, wrapped)

    spy("density_grad_raw")
    spy("appfeat_grad_raw")
    planes = f._render_params()[:13]
    # (a) only the points
    for p in planes:
        p.requires_grad_(False)
        p.grad = None
    try:
        x = _cu(q).requires_grad_(True)
        (f.lookup_density(x).sum() + f.lookup_appfeature(x).sum()).backward()
        assert x.grad is not None and all(p.grad is None for p in planes)
        assert sorted(seen) == [("appfeat_grad_raw", True, None), ("density_grad_raw", True, None)]
        # (b) one plane of each family and basis_mat, not the points
        seen.clear()
        planes[4].requires_grad_(True); planes[7].requires_grad_(True); planes[12].requires_grad_(True)
        x = _cu(q)
        out = f.lookup_density(x).sum() + f.lookup_appfeature(x).sum()
        g = torch.autograd.grad(out, [planes[4], planes[7], planes[12]])
        assert all(float(v.abs().max()) > 0 for v in g)
        want_d = [i == 4 for i in range(12)] + [False]
        want_a = [i == 7 for i in range(12)] + [True]
        assert sorted(seen) == [("appfeat_grad_raw", False, want_a), ("density_grad_raw", False, want_d)]
        # (c) nothing requires grad: the forward-only calls, no graph
        for p in planes:
            p.requires_grad_(False)
        assert not f.lookup_density(x).requires_grad and not f.lookup_appfeature(x).requires_grad
    finally:
        for p in planes:
            p.requires_grad_(True)
    with torch.no_grad():
        x = _cu(q).requires_grad_(True)
        assert not f.lookup_density(x).requires_grad and not f.lookup_appfeature(x).requires_grad
    assert not f.compute_appfeature(_cu(q).requires_grad_(True)).requires_grad
    # sigma follows by autograd through feature2density
    x = _cu(q).requires_grad_(True)
    gx, = torch.autograd.grad(f.feature2density(f.lookup_density(x)).sum(), x)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    # no second-order gradients
    for fn in (f.lookup_density, f.lookup_appfeature):
        x = _cu(q).requires_grad_(True)
        g1, = torch.autograd.grad(fn(x).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()
    for fn in (f.lookup_density, f.lookup_appfeature, f.compute_appfeature):
        with pytest.raises(_lib.NvfiError):
            fn(torch.from_numpy(q))
    m = make_model("A")[0]
    assert torch.equal(m.lookup_density(_cu(q)), f.lookup_density(_cu(q))) and torch.equal(m.compute_appfeature(_cu(q)), f.compute_appfeature(_cu(q)))
    assert m.lookup_appfeature(_cu(q).requires_grad_(True)).requires_grad


def test_print_worst():
    for k in sorted(WORST):
        print(f"[lookup] worst error / bound: {k}: {WORST[k]:.2f}")
