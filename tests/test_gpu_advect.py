"""Differentiable advection on the device - field.advect (nvfi_integrate_pos forward, nvfi_advect_grad backward; csrc/advect.hip) - against the float64
yardstick tests/advect64.py and the reference's goldens (tests/golden/advect.npz, advect_net_*.npz; tests/golden/make_golden_advect.py).

Bound per tensor (xk is compared bit for bit with integrate_pos; gx and the 12 net gradients with conftest.assert_grad): max(3 x the plain-fp32 floor
of the case, 1e-5).  The floor is the distance of advect64(float32) from advect64(float64) relative to the tensor's max - advect64.GOLDEN_FLOOR for
the golden cases (measured on the CPU), measured in the test by the same rule for the shape cases; 2e-8 .. 1.4e-6 everywhere, so the bound is 1e-5
throughout: B_SMALL of tests/test_gpu_render64.py, under which that file measured the device's velocity-net error on small lists at 1.3e-6 (the
render's figure, not this call's).  Every test prints error / floor per tensor.

Sensitivity (what a lost point or tile would do to the yardstick, N = 129 and 32 769, field A): dropping the last point of N = 129 moves every net
tensor by 7e-2 .. 2.4e-1 at one step - and by exactly nothing at three steps (T -> T - 1.3 ts), where that point's midpoint leaves the gate in its
first step and it never moves: BLIND.  The last 32-point tile of N = 32 769 holds one point, which starts outside the gate: BLIND at one and at
three steps.  The cases are asserted to BE blind so that the entries cannot outlive their reason, and N = 32 769 carries a second cut - the last 33
points, the ragged tile and the full one in front of it - which moves every net tensor by more than 2e-2."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import advect64 as a64
import flow64 as f64
import render64 as r64
from conftest import GOLD, assert_grad
from helpers import load_meta, make_model

pytestmark = pytest.mark.gpu

B_FLOOR = 1e-5
T = 19.0 / 60.0
GOLDEN = sorted(a64.GOLDEN_FLOOR)
SHAPES = (1, 31, 32, 33, 127, 128, 129, 257, 32769)
BLIND = {(129, 3, "last point"), (32769, 1, "last tile"), (32769, 3, "last tile")}


@pytest.fixture(scope="module")
def models():
    return {k: make_model(k)[0] for k in "AB"}


@pytest.fixture(scope="module")
def fields():
    out = {}
    for kind in "AB":
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        out[kind] = r64.Field(sd, meta)
    return out


@pytest.fixture(scope="module")
def adv_gold():
    return np.load(os.path.join(GOLD, "advect.npz"))


def _wparams(f):
    return f._render_params()[19:31]


def _device(model, x, g, t, t1, **kw):
    """value and gradients of sum(advect(x) * g) on the device: dict(xk, gx, <12 names>) as numpy, and the device tensors of xk / gx"""
    f = model.nvfi
    f.eval()
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(True)
    gt = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    y = f.advect(xt, t, t1, **kw)
    grads = torch.autograd.grad((y * gt).sum(), [xt] + list(_wparams(f)), allow_unused=True)
    out = dict(xk=y.detach().cpu().numpy(), gx=grads[0].cpu().numpy(), xk_dev=y.detach(), gx_dev=grads[0])
    for k, p, gr in zip(a64.NET_NAMES, _wparams(f), grads[1:]):
        out[k] = (torch.zeros_like(p) if gr is None else gr).cpu().numpy()
    return out


def _times(f, steps):
    ts = f.tmax / (f.num_keyframes - 1)
    return (T, T + ts / 4) if steps == 1 else (T, T - 1.3 * ts)


_yard = {}


def _yardstick(fields, kind, N, steps, f):
    """float64 and float32 yardstick of a shape case, computed once on the device and shared"""
    key = (kind, N, steps)
    if key not in _yard:
        x, g = a64.case_inputs(N)
        t, t1 = _times(f, steps)
        y64 = a64.advect64(fields[kind], x, t, t1, g, device="cuda")
        y32 = a64.advect64(fields[kind], x, t, t1, g, dtype=torch.float32, device="cuda")
        _yard[key] = (x, g, y64, a64.floors(y32, y64), y32)
    return _yard[key]


def _bounds(floor3):
    return dict(xk=max(3 * floor3[0], B_FLOOR), gx=max(3 * floor3[1], B_FLOOR), net=max(3 * floor3[2], B_FLOOR))


def _check_grads(dev, y64, floor3, label):
    b = _bounds(floor3)
    worst = 0.0
    for k in ("gx",) + tuple(a64.NET_NAMES):
        bound, floor = (b["gx"], floor3[1]) if k == "gx" else (b["net"], floor3[2])
        ref = y64[k]
        if np.abs(ref).max() == 0:
            assert not dev[k].any(), (label, k, "the yardstick's gradient is exactly zero")
            continue
        e = f64.rel_err(dev[k], ref)
        print(f"[advect] {label}: {k}: max |.| {np.abs(ref).max():.3g}, error {e:.2e}, fp32 floor {floor:.1e}, error / floor {e / floor if floor else float('inf'):.1f}, bound {bound:.1e}")
        assert_grad(dev[k], ref, bound, f"{label}:{k}")
        worst = max(worst, e)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. golden cases
@pytest.mark.parametrize("case", GOLDEN)
def test_golden_cases(models, fields, adv_gold, case):
    z, model = adv_gold, models[case[0]]
    f = model.nvfi
    x, g, t, t1 = z[case + ":x"], z[case + ":g"], float(z[case + ":t"]), float(z[case + ":t_target"])
    dev = _device(model, x, g, t, t1)
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        ref = f.integrate_pos(xt, torch.full((len(x),), t, device="cuda"), torch.full((len(x),), t1, device="cuda"))
        assert torch.equal(f.advect(xt, t, t1), ref)                     # the no-grad form IS integrate_pos
    assert torch.equal(dev["xk_dev"], ref), (case, "advect's value is integrate_pos' bit for bit")
    np.testing.assert_allclose(dev["xk"], z[case + ":xk"], rtol=1e-4, atol=1e-5)
    y64 = a64.advect64(fields[case[0]], x, t, t1, g)
    assert not y64["edge"].any() and len(y64["steps"]) == int(z[case + ":steps"]) and y64["n_rejected"] == int(z[case + ":n_rejected"])
    print(f"[advect] {case}: xk against float64 {f64.rel_err(dev['xk'], y64['xk']):.2e} (fp32 floor {a64.GOLDEN_FLOOR[case][0]:.1e})")
    if case.endswith("c0"):
        assert np.array_equal(dev["gx"], g) and all(not dev[k].any() for k in a64.NET_NAMES)
        return
    _check_grads(dev, y64, a64.GOLDEN_FLOOR[case], case)
    net = a64.golden_net(GOLD, case)         # ... and the reference's own fp32 gradients sit within the same bound of the device's
    for k in a64.NET_NAMES:
        assert f64.rel_err(dev[k], net[k]) < 2 * _bounds(a64.GOLDEN_FLOOR[case])["net"], (case, k)
    assert f64.rel_err(dev["gx"], z[case + ":gx"]) < 2 * _bounds(a64.GOLDEN_FLOOR[case])["gx"]


# ---------------------------------------------------------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("N", SHAPES)
def test_shapes(models, fields, N, steps):
    f = models["A"].nvfi
    x, g, y64, floor3, y32 = _yardstick(fields, "A", N, steps, f)
    assert len(y64["steps"]) == steps and not y64["edge"].any() and not y32["edge"].any()
    t, t1 = _times(f, steps)
    dev = _device(models["A"], x, g, t, t1)
    e = f64.rel_err(dev["xk"], y64["xk"])
    print(f"[advect] A:N={N}:{steps} step(s): xk error {e:.2e}, fp32 floor {floor3[0]:.1e}")
    assert e <= _bounds(floor3)["xk"]
    _check_grads(dev, y64, floor3, f"A:N={N}:{steps}")


def test_single_gated_point_is_the_identity(models, fields):
    """N = 1 on field B: the one point lies outside the surround box - exact identity, gx == g bitwise, every net gradient exactly zero"""
    f = models["B"].nvfi
    x, g = a64.case_inputs(1)
    t, t1 = _times(f, 3)
    y64 = a64.advect64(fields["B"], x, t, t1, g)
    assert y64["n_outside"] == 1 and y64["gated_all"].all() and len(y64["steps"]) == 3
    dev = _device(models["B"], x, g, t, t1)
    assert np.array_equal(dev["xk"], x) and np.array_equal(dev["gx"], g)
    assert all(not dev[k].any() for k in a64.NET_NAMES)


# ---------------------------------------------------------------------------------------------------------------- 3. sensitivity
@pytest.mark.parametrize("N,steps,what", [(129, 1, "last point"), (129, 3, "last point"), (32769, 1, "last tile"), (32769, 3, "last tile"),
                                          (32769, 1, "last two tiles"), (32769, 3, "last two tiles")])
def test_yardstick_sees_a_lost_tile(models, fields, N, steps, what):
    """the comparison of test_shapes can see a lost point / tile: cutting it out of the yardstick moves some net tensor by at least 3 x its bound -
    or the case is listed as BLIND, and is asserted to be"""
    f = models["A"].nvfi
    x, g, y64, floor3, _ = _yardstick(fields, "A", N, steps, f)
    keep = N - 1 if what == "last point" else (N - 1) // 32 * 32 if what == "last tile" else (N - 1) // 32 * 32 - 32
    t, t1 = _times(f, steps)
    cut = a64.advect64(fields["A"], x[:keep], t, t1, g[:keep], device="cuda")
    bound = _bounds(floor3)["net"]
    s = {k: f64.rel_err(cut[k], y64[k]) for k in a64.NET_NAMES}
    print(f"[advect] sensitivity N={N}, {steps} step(s), {what}: moves the net tensors by {min(s.values()):.2e} .. {max(s.values()):.2e} (3 x bound {3 * bound:.1e})")
    if (N, steps, what) in BLIND:
        assert not any(v >= 3 * bound for v in s.values()), (N, steps, what, "is listed as blind but is not", s)
    else:
        assert any(v >= 3 * bound for v in s.values()), (N, steps, what, s)


# ---------------------------------------------------------------------------------------------------------------- 4. chunking
def test_chunks(models, fields, adv_gold):
    model, case = models["A"], "A:c2"
    f, z = model.nvfi, adv_gold
    x, g, t, t1 = z[case + ":x"], z[case + ":g"], float(z[case + ":t"]), float(z[case + ":t_target"])
    one = _device(model, x, g, t, t1)
    assert f.last_advect_chunks == 1
    nb, desc = C.c_int64(0), f._desc()
    from nvfi_amd import _lib
    _lib.check(_lib.lib().nvfi_advect_grad_workspace_bytes(C.byref(desc), C.c_int64(128), C.c_float(t), C.c_float(t1), C.byref(nb)))
    three = _device(model, x, g, t, t1, max_workspace_bytes=nb.value + 4096)      # room for one 128-point group: 128 + 128 + 1
    assert f.last_advect_chunks == 3 and f.last_advect_workspace_bytes <= nb.value + 4096
    assert torch.equal(one["gx_dev"], three["gx_dev"]) and torch.equal(one["xk_dev"], three["xk_dev"])
    y64 = a64.advect64(fields["A"], x, t, t1, g)
    _check_grads(one, y64, a64.GOLDEN_FLOOR[case], case + ":one chunk")
    _check_grads(three, y64, a64.GOLDEN_FLOOR[case], case + ":three chunks")
    with pytest.raises(_lib.NvfiError):
        _device(model, x, g, t, t1, max_workspace_bytes=1 << 20)


# ---------------------------------------------------------------------------------------------------------------- 5. zero steps and refusal
def test_zero_steps_and_refusal(models):
    from nvfi_amd import _lib
    model = models["A"]
    f = model.nvfi
    x, g = a64.case_inputs(129)
    dev = _device(model, x, g, T, T)
    assert np.array_equal(dev["xk"], x) and np.array_equal(dev["gx"], g) and all(not dev[k].any() for k in a64.NET_NAMES)
    ts = f.tmax / (f.num_keyframes - 1)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    with pytest.raises(_lib.NvfiError, match="error 2"):
        f.advect(xt, 0.0, 32.25 * ts)                                # 65 steps: refused, not truncated
    with torch.no_grad(), pytest.raises(_lib.NvfiError, match="error 2"):
        f.advect(xt, 0.0, 32.25 * ts)
    assert f.advect(xt, 0.0, 31.75 * ts).shape == xt.shape             # 64 steps run
    desc, gt, gx = f._desc(), torch.from_numpy(g).cuda(), torch.empty(129, 3, device="cuda")
    G = f._grads_struct_vel([None] * 24)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().nvfi_advect_grad(C.byref(desc), C.c_int64(129), _lib.ptr(xt.detach()), C.c_float(0.0), C.c_float(32.25 * ts), _lib.ptr(gt), _lib.ptr(gx),
                                     C.byref(G), _lib.ptr(ws), C.c_int64(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 2 and b"more than 64 RK2 steps" in _lib.lib().nvfi_last_error()
    rc = _lib.lib().nvfi_advect_grad(C.byref(desc), C.c_int64(129), _lib.ptr(xt.detach()), C.c_float(T), C.c_float(T + ts / 4), _lib.ptr(gt), _lib.ptr(gx),
                                     C.byref(G), _lib.ptr(ws), C.c_int64(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 4                                                    # a workspace that is too small is refused before anything is launched
    # out of scope: per-point times with a gradient, the fp16-input modes
    tt = torch.linspace(0.1, 0.2, 129, device="cuda")
    with pytest.raises(NotImplementedError):
        f.advect(xt, tt, tt + 0.1)
    with torch.no_grad():
        assert torch.equal(f.advect(xt, tt, tt + 0.1), f.integrate_pos(xt, tt, tt + 0.1))
    f.vel_fp16 = 1
    try:
        with pytest.raises(NotImplementedError):
            f.advect(xt, T, T + ts / 4)
    finally:
        f.vel_fp16 = False


# ---------------------------------------------------------------------------------------------------------------- 6. repeat
def test_repeat(models, adv_gold):
    """two backward calls on the same inputs: gx bit for bit; the net gradients too - the ring kernel walks a fixed, strided set of tiles per slab
    and k_wgrad_reduce sums the slabs in a fixed order, one atomic add per element into a zeroed buffer"""
    z, case = adv_gold, "B:c3"
    x, g, t, t1 = z[case + ":x"], z[case + ":g"], float(z[case + ":t"]), float(z[case + ":t_target"])
    a = _device(models["B"], x, g, t, t1)
    b = _device(models["B"], x, g, t, t1)
    assert torch.equal(a["gx_dev"], b["gx_dev"])
    same = {k: bool(np.array_equal(a[k], b[k])) for k in a64.NET_NAMES}
    print(f"[advect] repeat: net gradients identical: {same}")
    assert all(same.values()), same


# ---------------------------------------------------------------------------------------------------------------- 7. gate / rejection
def test_gated_points_pass_their_gradient_through(models, fields, adv_gold):
    z, case = adv_gold, "B:c2"
    x, g, t, t1 = z[case + ":x"], z[case + ":g"], float(z[case + ":t"]), float(z[case + ":t_target"])
    y64 = a64.advect64(fields["B"], x, t, t1, g)
    ga = y64["gated_all"]
    assert ga.sum() == 98 and y64["n_rejected"] == 8
    dev = _device(models["B"], x, g, t, t1)
    assert np.array_equal(dev["gx"][ga], g[ga]) and np.array_equal(dev["xk"][ga], x[ga])
    assert not np.array_equal(dev["gx"][~ga], g[~ga])


# ---------------------------------------------------------------------------------------------------------------- 8. replay
def test_replay_three_adam_iterations(adv_gold):
    z = adv_gold
    model, _ = make_model("A")
    f = model.nvfi
    f.eval()
    x, target = torch.from_numpy(z["replay:x"]).cuda(), torch.from_numpy(z["replay:target"]).cuda()
    t, t1 = float(z["replay:t"]), float(z["replay:t_target"])
    opt = torch.optim.Adam(f.vel_net.weight_net.parameters(), lr=1e-3)
    for it in range(3):
        opt.zero_grad()
        loss = ((f.advect(x, t, t1) - target) ** 2).mean()
        loss.backward()
        opt.step()
        print(f"[advect] replay iteration {it}: loss {float(loss):.8g}, reference {float(z['replay:loss'][it]):.8g}")
        np.testing.assert_allclose(float(loss), float(z["replay:loss"][it]), rtol=2e-4, err_msg=f"iteration {it}")
    # as tests/test_gpu_training_loop.py: the bulk agrees to 1e-3 of the distance moved, nothing differs by more than three steps can move an element
    start = {k[3:]: v for k, v in np.load(os.path.join(GOLD, "field_A.npz")).items() if k.startswith("sd:")}
    sd = model.state_dict()
    for name in a64.NET_NAMES:
        ref, got = z["replay:" + name].astype(np.float64), sd["nvfi." + name].detach().cpu().contiguous().numpy().astype(np.float64)
        moved = np.abs(ref - start["nvfi." + name].astype(np.float64))
        err = np.abs(got - ref)
        assert moved.max() > 0 and err.max() <= 3.1 * 1e-3, (name, err.max(), moved.max())
        frac_bad = np.mean(err > 1e-3 * moved.max() + 1e-7)
        assert frac_bad < 0.02, (name, frac_bad, err.max(), moved.max())


# ---------------------------------------------------------------------------------------------------------------- 9. untouched
def test_nothing_else_is_touched(adv_gold, gold):
    from nvfi_amd.models import Ray, Renderer
    z, case = adv_gold, "A:c2"
    model, _ = make_model("A")
    f = model.nvfi
    o, d = torch.from_numpy(gold["A:rays_o"]).cuda(), torch.from_numpy(gold["A:rays_d"]).cuda()
    ren = Renderer(model, 0, 0, 2048)
    u = torch.rand(o.shape[0], 1, generator=torch.Generator().manual_seed(3))

    def render():
        model.train(); ren.train()
        f.jitter_override = u.clone()
        try:
            out = ren.render(T, Ray(o, d, 0, 1), white_background=True, mode="train")
        finally:
            f.jitter_override = None
        return [m.detach().clone() for m in out[:4]]

    before = render()
    model.eval()
    x = torch.from_numpy(z[case + ":x"]).cuda().requires_grad_(True)
    y = f.advect(x, float(z[case + ":t"]), float(z[case + ":t_target"]))
    (y * torch.from_numpy(z[case + ":g"]).cuda()).sum().backward()
    assert x.grad is not None and all(p.grad is not None and bool(p.grad.abs().max() > 0) for p in f.vel_net.weight_net.parameters())
    assert all(p.grad is None for p in f.vel_net.a_weight_net.parameters())
    planes = list(f.density_plane_space) + list(f.density_plane_time) + list(f.app_plane_space) + list(f.app_plane_time)
    assert all(p.grad is None for p in planes) and f.basis_mat.weight.grad is None
    assert all(p.grad is None for p in f.renderModule.parameters())
    with pytest.raises(RuntimeError):            # once_differentiable: no second-order gradients
        x2 = torch.from_numpy(z[case + ":x"]).cuda().requires_grad_(True)
        gx, = torch.autograd.grad(f.advect(x2, T, T + 0.05).sum(), x2, create_graph=True)
        gx.sum().backward()
    after = render()
    for a, b in zip(before, after):
        assert torch.equal(a, b), "a training render around an advect backward gives the same maps bit for bit"
