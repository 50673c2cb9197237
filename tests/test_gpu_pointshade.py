"""Differentiable point shading on the device - nvfi_render_mlp_grad (csrc/point_shade.hip), its raw wrapper (utils/field_lookup.py:
render_mlp_grad_raw) and field.shade / lookup_rgb - against the float64 yardstick tests/pointshade64.py, which tests/test_pointshade_golden.py pins
to the reference's goldens.  The yardsticks run in torch on the GPU.

Fields: A, B (A's render MLP on other inputs), D (A's geometry with SH shading: app_dim 27, no MLP).  Bound of every comparison, the same for every
tensor (rgb, g_features, g_xyz, g_view, the six MLP gradients): |got - ref64| <= max(3 x floor, 1e-5 x max |ref64|), floor = the yardstick's float32
evaluation against its float64 evaluation on that case (lookup64.bound).  Every check prints `[pointshade] <case>: <tensor>: error / bound`.  The
inputs of every yardstick case come from the seeds test_pointshade_golden.py lists and checks (no ReLU within 64 float32 floors of zero): no point
is masked out.

Measured on an MI355X, worst error / bound over all cases (test_print_worst prints them): rgb 0.03, g_features 0.04, g_xyz 0.05,
g_view 0.04, the six MLP gradients 0.01 - 0.04: the bounds are the 1e-5 x max term everywhere, the errors sit at the float32 floor.  Two calls and a
hipGraph replay are bit-identical in every output, the weight gradients included.  The file takes 5 s."""
import numpy as np
import pytest
import torch

import advect64 as a64
import lookup64 as l64
import point64 as p64
import pointshade64 as s64
from helpers import field_state, make_model
from test_pointshade_golden import CHUNK_N, KINDS, SEEDS, SIZES

pytestmark = pytest.mark.gpu
SENT = -7.0
WORST = {}
MLP = slice(13, 19)


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


_yard = {}


def _case(dev, kind, N):
    """inputs of the listed seed and the (float64, float32) yardstick tensors of the case, computed once"""
    if (kind, N) not in _yard:
        yf = dev[kind][1]
        a = s64.inputs(yf, N, SEEDS[(kind, N)])
        _yard[(kind, N)] = (a, s64.tensors(s64.shade64(yf, *a, device="cuda")), s64.tensors(s64.shade64(yf, *a, dtype=torch.float32, device="cuda")))
    return _yard[(kind, N)]


def _buffers(f, which=None, fill=0.0):
    """gradient buffers of the six MLP tensors (None where not asked for; none at all under SH) and the nvfi_grads that points at them"""
    params = f._render_params()[MLP]
    if params[0] is None:
        return [], None
    bufs = [torch.full_like(p, fill) if (which is None or n in which) else None for n, p in zip(s64.MLP_NAMES, params)]
    return bufs, f._grads_struct([None] * MLP.start + bufs)


def _raw(f, a, outs=(True, True, True), which=None, bufs=None, ws=None):
    """one raw call -> {label: numpy} in pointshade64.tensors' labels (without rgb), the three device tensors, the buffers"""
    if bufs is None:
        bufs, G = _buffers(f, which)
    else:
        G = f._grads_struct([None] * MLP.start + bufs) if bufs else None
    xyz, view, feat, g = [_cu(v) if isinstance(v, np.ndarray) else v for v in a]
    o = _fl().render_mlp_grad_raw(f._desc(), xyz, view, feat, g, g_features=outs[0], g_xyz=outs[1], g_view=outs[2], grads=G, workspace=ws)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in zip(("g_features", "g_xyz", "g_view"), o) if v is not None}
    got.update({"grad:" + n: b.cpu().numpy() for n, b in zip(s64.MLP_NAMES, bufs) if b is not None})
    return got, o, bufs


def _check(label, got, t64, t32):
    """every tensor of `got` inside the bound of its yardstick entry; prints error / bound"""
    for k, v in got.items():
        ref = t64[k]
        b = s64.bound(ref, t32[k])
        assert np.asarray(v).shape == ref.shape, (label, k, np.asarray(v).shape, ref.shape)
        e = s64.max_err(v, ref)
        ratio = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        print(f"[pointshade] {label}: {k}: max |ref64| {np.abs(ref).max() if ref.size else 0:.3g}, error {e:.2e}, float32 floor {s64.max_err(t32[k], ref):.2e}, "
              f"bound {b:.2e}, error / bound {ratio:.2f}", flush=True)
        key = k.replace("grad:renderModule.", "") + ":" + label.split(":")[0]
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        assert e <= b, (label, k, e, b, ratio)


# ---------------------------------------------------------------------------------------------------------------- 1. the raw call
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_raw_against_yardstick(dev, kind, N):
    f = dev[kind][0]
    a, t64, t32 = _case(dev, kind, N)
    rgb = f._render_module_call(_cu(a[0]), _cu(a[1]), _cu(a[2]))
    _check(f"{kind}:N={N}", {"rgb": rgb.cpu().numpy()}, t64, t32)
    got, _, _ = _raw(f, a)
    assert set(got) == set(t64) - {"rgb"} and len(got) == (3 if kind == "D" else 9)
    _check(f"{kind}:N={N}", got, t64, t32)
    if kind == "D":
        assert not got["g_xyz"].any()


@pytest.mark.parametrize("kind", KINDS)
def test_null_outputs_and_members(dev, kind):
    """NULL g_* outputs and NULL grads members (or grads == NULL) leave sentinel-filled buffers untouched; what is asked for is unchanged by it"""
    f = dev[kind][0]
    a, t64, t32 = _case(dev, kind, 33)
    full, o_full, _ = _raw(f, a)
    d = int(f.app_dim)
    for skip in range(3):
        sent = [torch.full(s, SENT, device="cuda") for s in ((33, d), (33, 3), (33, 3))]
        outs = [None if k == skip else True for k in range(3)]
        part, o, _ = _raw(f, a, outs=outs)
        assert o[skip] is None and all(torch.equal(o[k], o_full[k]) for k in range(3) if k != skip)
        # the same through caller-owned tensors: the skipped one keeps its sentinel (it is not passed), the others are overwritten
        _, o2, _ = _raw(f, a, outs=[None if k == skip else sent[k] for k in range(3)])
        assert all(o2[k] is sent[k] and torch.equal(sent[k], o_full[k]) for k in range(3) if k != skip)
        assert bool((sent[skip] == SENT).all())
    if kind == "D":
        return
    for which in (["renderModule.mlp.0.weight"], ["renderModule.mlp.2.bias", "renderModule.mlp.4.weight"], []):
        bufs, _ = _buffers(f, fill=SENT)
        params = f._render_params()[MLP]
        live = [torch.zeros_like(p) if n in which else None for n, p in zip(s64.MLP_NAMES, params)]
        got, _, _ = _raw(f, a, bufs=live)
        assert {k for k in got if k.startswith("grad:")} == {"grad:" + n for n in which}
        _check(f"{kind}:members {len(which)}", got, t64, t32)
        for n in which:
            assert np.array_equal(got["grad:" + n], full["grad:" + n]), n
        assert all(bool((b == SENT).all()) for b in bufs)
    # grads == NULL
    xyz, view, feat, g = [_cu(v) for v in a]
    o = _fl().render_mlp_grad_raw(f._desc(), xyz, view, feat, g, g_view=True, grads=None)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(o, o_full))
    # buffers that hold values are accumulated into
    first, _, bufs = _raw(f, a)
    second, _, _ = _raw(f, a, bufs=bufs)
    for n in s64.MLP_NAMES:
        assert s64.max_err(second["grad:" + n] / 2.0, first["grad:" + n]) <= 1e-6 * np.abs(first["grad:" + n]).max()


def test_empty_call_and_errors(dev):
    from nvfi_amd import _lib
    f = dev["A"][0]
    fl = _fl()
    desc = f._desc()
    bufs, G = _buffers(f, fill=SENT)
    e3, e32 = torch.empty(0, 3, device="cuda"), torch.empty(0, 32, device="cuda")
    o = fl.render_mlp_grad_raw(desc, e3, e3, e32, e3, g_view=True, grads=G)
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in o] == [(0, 32), (0, 3), (0, 3)] and all(bool((b == SENT).all()) for b in bufs)
    assert f.shade(e3, e3, e32.requires_grad_(True)).shape == (0, 3)
    a, _, _ = _case(dev, "A", 33)
    need = fl.render_mlp_grad_workspace_bytes(desc, 33)
    # the stash grows by whole 128-point workgroups, the packed points (2 x 16 B) by the point
    assert fl.render_mlp_grad_workspace_bytes(desc, 128) - need == 2 * (128 * 16 - 3 * 256)
    assert fl.render_mlp_grad_workspace_bytes(desc, 129) - need > 4 * (224 + 160) * 256
    outs = [torch.full(s, SENT, device="cuda") for s in ((33, 32), (33, 3), (33, 3))]
    with pytest.raises(_lib.NvfiError, match="error 4"):
        _raw(f, a, outs=outs, bufs=bufs, ws=torch.empty(need - 256, dtype=torch.uint8, device="cuda"))
    bad = f._desc()
    bad.Cd = 16
    with pytest.raises(_lib.NvfiError, match="error 2"):
        fl.render_mlp_grad_raw(bad, *[_cu(v) for v in a], grads=G)
    L = _lib.lib()
    import ctypes as C
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    x = _cu(a[0])
    rc = L.nvfi_render_mlp_grad(C.byref(desc), C.c_int64(33), _lib.ptr(x), None, _lib.ptr(x), _lib.ptr(x), None, None, None, None, _lib.ptr(ws),
                                C.c_int64(need), None)
    assert rc == 2
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all()) for b in bufs + outs), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------------------------- 2. repeats
@pytest.mark.parametrize("kind", ("A", "D"))
def test_repeats_and_graph_replay(dev, kind):
    """two calls and one hipGraph replay: g_features / g_xyz / g_view bit for bit, and so are the weight gradients - the ring's items are dealt to
    its workers by index, the reduce sums the slabs in a fixed order and adds each entry once into a cleared buffer"""
    f = dev[kind][0]
    fl = _fl()
    a, t64, t32 = _case(dev, kind, 257)
    r1, o1, _ = _raw(f, a)
    r2, o2, _ = _raw(f, a)
    assert all(torch.equal(x, y) for x, y in zip(o1, o2))
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), (k, "two calls", s64.max_err(r1[k], r2[k]))
    desc = f._desc()
    ins = [_cu(v) for v in a]
    d = int(f.app_dim)
    outs = [torch.full(s, SENT, device="cuda") for s in ((257, d), (257, 3), (257, 3))]
    bufs, G = _buffers(f)
    ws = torch.empty(fl.render_mlp_grad_workspace_bytes(desc, 257), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        fl.render_mlp_grad_raw(desc, *ins, g_features=outs[0], g_xyz=outs[1], g_view=outs[2], grads=G, workspace=ws)
    torch.cuda.current_stream().wait_stream(cap)
    for t in bufs:
        t.zero_()
    for t in outs:
        t.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, o1)), "per-point gradients of the replay"
    got = {"grad:" + n: b.cpu().numpy() for n, b in zip(s64.MLP_NAMES, bufs)}
    _check(f"{kind}:N=257 replay", got, t64, t32)
    for k in got:
        assert np.array_equal(got[k], r1[k]), (k, "replay", s64.max_err(got[k], r1[k]))


# ---------------------------------------------------------------------------------------------------------------- 3. chunks
@pytest.mark.parametrize("kind", ("A", "D"))
def test_chunked_backward(dev, kind):
    """N = 385 through field.shade with a workspace limit that admits one 128-point group: four chunks; per-point gradients bit for bit those of
    the unchunked raw call, weight gradients (summed in another order) within the bound"""
    f = dev[kind][0]
    fl = _fl()
    a, t64, t32 = _case(dev, kind, CHUNK_N)
    whole, o, _ = _raw(f, a)
    _check(f"{kind}:N={CHUNK_N} whole", whole, t64, t32)
    limit = fl.render_mlp_grad_workspace_bytes(f._desc(), 128)
    assert limit < fl.render_mlp_grad_workspace_bytes(f._desc(), 256)
    x, v, fe = [_cu(t).requires_grad_(True) for t in a[:3]]
    params = [p for p in f._render_params()[MLP] if p is not None]
    rgb = f.shade(x, v, fe, max_workspace_bytes=limit)
    grads = torch.autograd.grad((rgb * _cu(a[3])).sum(), [fe, x, v] + params)
    torch.cuda.synchronize()
    assert f.last_shade_chunks == 4 and f.last_shade_workspace_bytes == limit
    assert all(torch.equal(g, w) for g, w in zip(grads[:3], o)), "per-point gradients do not depend on the chunking"
    got = {"grad:" + n: g.cpu().numpy() for n, g in zip(s64.MLP_NAMES, grads[3:])}
    _check(f"{kind}:N={CHUNK_N} four chunks", got, t64, t32)
    rgb2 = f.shade(x, v, fe)
    torch.autograd.grad(rgb2.sum(), fe)
    assert f.last_shade_chunks == 1


# ---------------------------------------------------------------------------------------------------------------- 4. autograd surface
@pytest.mark.parametrize("kind", ("A", "D"))
def test_autograd_surface(dev, kind, monkeypatch):
    from nvfi_amd import _lib
    f = dev[kind][0]
    fl = _fl()
    a, t64, t32 = _case(dev, kind, 129)
    xyz, view, feat, g = [_cu(v) for v in a]
    with torch.no_grad():
        ref = f.renderModule(xyz, view, feat, {}) if kind == "A" else f._render_module_call(xyz, view, feat)
        assert torch.equal(f.shade(xyz, view, feat.clone().requires_grad_(True)), ref)
    fe = feat.clone().requires_grad_(True)
    rgb = f.shade(xyz, view, fe)
    assert rgb.requires_grad and rgb.shape == (129, 3) and torch.equal(rgb.detach(), ref), "shade's value is renderModule's bit for bit"
    seen = []
    real = fl.render_mlp_grad_raw

    def spy(desc, x, v, ft, gr, g_features=True, g_xyz=True, g_view=None, grads=None, workspace=None):
        ptrs = None if grads is None else [bool(p) for pair in zip(grads.rW, grads.rb) for p in pair]
        seen.append((g_features is not None, g_xyz is not None, g_view is not None, ptrs))
        return real(desc, x, v, ft, gr, g_features=g_features, g_xyz=g_xyz, g_view=g_view, grads=grads, workspace=workspace)
    monkeypatch.setattr(fl, "render_mlp_grad_raw", spy)
    params = [p for p in f._render_params()[MLP] if p is not None]
    for p in params:
        p.grad = None
    # (a) everything: .backward() fills the three inputs and the six MLP tensors
    x, v, fe = xyz.clone().requires_grad_(True), view.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    (f.shade(x, v, fe) * g).sum().backward()
    got = {"g_features": fe.grad.cpu().numpy(), "g_xyz": x.grad.cpu().numpy(), "g_view": v.grad.cpu().numpy()}
    got.update({"grad:" + n: p.grad.cpu().numpy() for n, p in zip(s64.MLP_NAMES, params)})
    _check(f"{kind}:autograd", got, t64, t32)
    assert seen == [(True, True, True, [True] * 6 if params else None)]
    for p in params:
        p.grad = None
        p.requires_grad_(False)
    try:
        # (b) only the view direction
        seen.clear()
        v = view.clone().requires_grad_(True)
        (f.shade(xyz, v, feat) * g).sum().backward()
        assert seen == [(False, False, True, None)] and torch.equal(v.grad, _cu(got["g_view"])) and all(p.grad is None for p in params)
        if params:
            # (c) the features and one weight, one bias
            seen.clear()
            params[2].requires_grad_(True); params[5].requires_grad_(True)
            fe = feat.clone().requires_grad_(True)
            (f.shade(xyz, view, fe) * g).sum().backward()
            assert seen == [(True, False, False, [False, False, True, False, False, True])]
            assert [p.grad is not None for p in params] == [False, False, True, False, False, True]
            assert np.array_equal(params[2].grad.cpu().numpy(), got["grad:" + s64.MLP_NAMES[2]])
            params[2].grad = params[5].grad = None
            params[2].requires_grad_(False); params[5].requires_grad_(False)
        # (d) nothing requires grad: the forward-only call, no graph
        assert not f.shade(xyz, view, feat).requires_grad
    finally:
        for p in params:
            p.requires_grad_(True)
    # once differentiable
    fe = feat.clone().requires_grad_(True)
    g1, = torch.autograd.grad(f.shade(xyz, view, fe).sum(), fe, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    with pytest.raises(_lib.NvfiError):
        f.shade(xyz.cpu(), view.cpu(), feat.cpu())
    if kind == "A":
        m = make_model("A")[0]
        assert torch.equal(m.shade(xyz, view, feat), ref) and m.shade(xyz, view, feat.clone().requires_grad_(True)).requires_grad


# ---------------------------------------------------------------------------------------------------------------- 5. lookup_rgb
def _points(f, N, seed):
    rng = np.random.default_rng(seed)
    grid, K = [int(v) for v in f.gridSize.tolist()], int(f.num_keyframes)
    q = l64.point_mix(rng, N, grid, K, extent=0.95, n_nodes=0)
    v = rng.standard_normal((N, 3))
    return q, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)


@pytest.mark.parametrize("kind", ("A", "D"))
def test_lookup_rgb(dev, kind):
    """value: renderModule(xyz, view, compute_appfeature(xyzt)) bit for bit, app_at within the bound.  Gradients: those of chaining
    render_mlp_grad_raw into appfeat_grad_raw by hand - xyzt bit for bit at N = 129; the planes and basis_mat, float atomics whose sums depend on
    the order of arrival, bit for bit at N = 2, where no sum has more than two addends, and within lookup64's bound of each other at N = 129"""
    f, yf = dev[kind]
    fl = _fl()
    app = f._render_params()[6:13]
    for N in (129, 2):
        q, view, g = _points(f, N, 61)
        qt, vt, gt = _cu(q), _cu(view), _cu(g)
        feat = f.compute_appfeature(qt)
        with torch.no_grad():
            val = f._render_module_call(qt[:, :3], vt, feat)
            assert torch.equal(f.lookup_rgb(qt, vt), val)
        y64, y32 = [p64.app64(yf, q, view, dtype=dt, device="cuda")["rgb"] for dt in (torch.float64, torch.float32)]
        _check(f"{kind}:lookup_rgb N={N}", {"rgb": val.cpu().numpy()}, {"rgb": y64}, {"rgb": y32})
        _check(f"{kind}:app_at N={N}", {"rgb": f.app_at(qt, vt).cpu().numpy()}, {"rgb": y64}, {"rgb": y32})
        x = qt.clone().requires_grad_(True)
        rgb = f.lookup_rgb(x, vt)
        assert torch.equal(rgb.detach(), val)
        grads = torch.autograd.grad((rgb * gt).sum(), [x] + list(app))
        # by hand
        desc = f._desc()
        gf, gx, _ = fl.render_mlp_grad_raw(desc, qt[:, :3], vt, feat, gt)
        bufs = [torch.zeros_like(p) for p in app]
        gq = fl.appfeat_grad_raw(desc, qt, gf, grads=f._grads_struct([None] * 6 + bufs))
        hand = gq.clone()
        hand[:, :3] += gx
        torch.cuda.synchronize()
        assert torch.equal(grads[0], hand), (N, "xyzt")
        assert float(grads[0][:, 3].abs().max()) > 0 and (kind == "D" or float(gx.abs().max()) > 0)
        if N == 2:
            assert all(torch.equal(a, b) for a, b in zip(grads[1:], bufs)), "planes and basis_mat"
        else:
            gfn = gf.cpu().numpy()
            t64 = l64.tensors(l64.app_lookup64(yf, q, gfn, device="cuda"))
            t32 = l64.tensors(l64.app_lookup64(yf, q, gfn, dtype=torch.float32, device="cuda"))
            for n, a, b in zip(l64.A_NAMES, grads[1:], bufs):
                assert l64.max_err(a.cpu().numpy(), b.cpu().numpy()) <= l64.bound(t64["grad:" + n], t32["grad:" + n]), n
                assert float(a.abs().max()) > 0


def test_chain_through_advect(dev):
    """q = cat(advect(x, t, t_k), t'_k) -> lookup_rgb -> a weighted sum -> backward: x.grad and the twelve weight_net gradients are, bit for bit,
    advect's backward fed the raw calls' g_xyz + g_xyzt[:, :3] by hand"""
    f, yf = dev["A"]
    fl = _fl()
    N = 129
    ts = f.tmax / (f.num_keyframes - 1)
    t, tk = 19.0 / 60.0, float(np.float32(ts))
    tnk = float(f.normalize_time_coord(torch.tensor([tk]))[0])
    x, _ = a64.case_inputs(N)
    _, view, g = _points(f, N, 71)
    vt, gt = _cu(view), _cu(g)
    wparams = f._render_params()[19:31]
    xt = _cu(x).requires_grad_(True)
    col = torch.full((N, 1), tnk, device="cuda")
    qx = torch.cat([f.advect(xt, t, tk), col], 1)
    grads = torch.autograd.grad((f.lookup_rgb(qx, vt) * gt).sum(), [xt] + list(wparams))
    # by hand
    x2 = _cu(x).requires_grad_(True)
    xk = f.advect(x2, t, tk)
    q = torch.cat([xk.detach(), col], 1)
    assert torch.equal(q, qx.detach())
    desc = f._desc()
    gf, gx, _ = fl.render_mlp_grad_raw(desc, q[:, :3], vt, f.compute_appfeature(q), gt)
    gq = fl.appfeat_grad_raw(desc, q, gf)
    hand = torch.autograd.grad(xk, [x2] + list(wparams), grad_outputs=(gx + gq[:, :3]).contiguous())
    assert torch.equal(grads[0], hand[0]), "x.grad is advect's backward of g_xyz + g_xyzt[:, :3]"
    assert all(torch.equal(a, b) for a, b in zip(grads[1:], hand[1:])), "the weight_net gradients are advect's backward of g_xyz + g_xyzt[:, :3]"
    assert float(grads[0].abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in grads[1:])


def test_print_worst():
    for k in sorted(WORST):
        print(f"[pointshade] worst error / bound: {k}: {WORST[k]:.2f}")
