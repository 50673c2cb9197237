"""Optical-flow supervision on the device - field.flow_loss, render_mse_backward_(target_flow=), render_test_evaluation(gt_flows=)
(nvfi_flow_loss_fwd / nvfi_flow_loss_bwd; csrc/flowloss.hip) - against the float64 yardstick tests/flowloss64.py on the device's OWN weights.

Bound per tensor (flow2d, g_weights and the 12 net gradients through conftest.assert_grad, the loss as a relative error): max(3 x the plain-fp32
floor, 1e-5).  The floor is the distance of flowloss64(float32) from flowloss64(float64) on the same inputs, relative to the tensor's max, measured
in the test and not taken below one fp32 ulp.  Every comparison prints error / bound and error / floor.

Rays: the golden rays of the hot-path fixture and grazing rays from the same camera position (short chords, the recipe of tests/test_gpu_flow.py),
rendered once in training mode with a fixed per-ray jitter; every case ends in a ray that looks away from the box (no masked sample: exact zeros)
and, from R = 7 up, starts with the pool's ray of fewest masked samples (one, asserted), carries one ray switched off by `valid` and one with a
NaN target.

Sensitivity: dropping the LAST masked entry (a list whose length is no multiple of 32) from the yardstick must move some net gradient by more than
the bound; a case where it does not is listed in BLIND and asserted to be blind."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import flow64 as f64
import flowloss64 as fl64
import render64 as r64
from conftest import GOLD, assert_grad
from helpers import field_state, make_model

pytestmark = pytest.mark.gpu

B_FLOOR = 1e-5
T = 19.0 / 60.0
SHAPES = (1, 2, 7, 64, 65, 257)
BLIND = set()


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _make_ctx(gold, kinds="AB"):
    flow_gold = np.load(os.path.join(GOLD, "flow.npz"))
    out = {}
    for kind in kinds:
        model, meta = make_model(kind)
        f = model.nvfi
        cam = (flow_gold[f"{kind}:pose"], int(flow_gold[f"{kind}:H"]), int(flow_gold[f"{kind}:W"]), float(flow_gold[f"{kind}:focal"]))
        out[kind] = dict(model=model, f=f, field=r64.Field(*field_state(model)), o=gold[f"{kind}:rays_o"], d=gold[f"{kind}:rays_d"], cam=cam,
                         ts=f.tmax / (f.num_keyframes - 1))
    return out


@pytest.fixture(scope="module")
def ctx(gold):
    return _make_ctx(gold)


def _wparams(f):
    return f._render_params()[19:31]


def _render(c, o, d, jit, t=T):
    """one TRAINING render with the given per-ray jitter -> the field's outputs (weights carries the autograd node)"""
    f = c["f"]
    c["model"].train()
    f.jitter_override = torch.from_numpy(np.ascontiguousarray(jit, dtype=np.float32)).reshape(-1, 1)
    try:
        return f(t, _cu(o), _cu(d), True)
    finally:
        f.jitter_override = None


_pools = {}


def _pool(c, kind, n=512):
    """the golden rays and n grazing rays with a fixed jitter each, and the device's masked count per ray of one training render of them all"""
    if kind not in _pools:
        rng = np.random.default_rng(11)
        ab = c["field"].aabb.numpy().astype(np.float64)
        q = rng.uniform(-1, 1, (n, 3))
        ax = rng.integers(0, 3, n)
        q[np.arange(n), ax] = np.sign(q[np.arange(n), ax]) * rng.uniform(0.97, 1.0, n)
        q[np.arange(n), (ax + 1) % 3] = np.sign(q[np.arange(n), (ax + 1) % 3]) * rng.uniform(0.9, 1.03, n)
        dg = (q + 1) / 2 * (ab[1] - ab[0]) + ab[0] - c["o"][0]
        o = np.concatenate([c["o"], np.tile(c["o"][:1], (n, 1))]).astype(np.float32)
        d = np.concatenate([c["d"], dg / np.linalg.norm(dg, axis=1, keepdims=True)]).astype(np.float32)
        jit = rng.random(len(o)).astype(np.float32)
        with torch.no_grad():
            w = _render(c, o, d, jit)[3].cpu().numpy()
        counts = (w > np.float32(c["field"].thres)).sum(1)
        _pools[kind] = (o, d, jit, counts)
        print(f"[flowloss] pool {kind}: masked per ray: golden mean {counts[:256].mean():.1f}, grazing rays with 1 sample: {(counts[256:] == 1).sum()}, "
              f"with 2: {(counts[256:] == 2).sum()}")
    return _pools[kind]


def _case(c, kind, R):
    """rays, jitter, target, valid of the case of R rays"""
    po, pd, pj, counts = _pool(c, kind)
    single = int(np.nonzero(counts == 1)[0][0])
    idx = list(range(100, 100 + R))                          # (ray 100 hits the object)
    idx = [i % 256 for i in idx]
    if R >= 7:
        idx[0] = single
    o, d, jit = po[idx].copy(), pd[idx].copy(), pj[idx].copy()
    if R >= 2:
        d[-1] = -d[-1]                                       # looks away from the box: nothing valid, nothing masked
    rng = np.random.default_rng(5 + R)
    target = rng.standard_normal((R, 2)).astype(np.float32)
    valid = np.ones(R, np.uint8)
    if R >= 7:
        valid[1] = 0
        target[2, 0] = np.nan
    return o, d, jit, target, valid


def _device(c, o, d, jit, dt, target, valid=None, kind="l2", delta=1.0, **kw):
    """value and gradients on the device: dict(flow2d, loss, n, g_weights, <12 names>) as numpy + the device tensors under *_dev"""
    f = c["f"]
    out = _render(c, o, d, jit)
    weights = out[3]
    v = None if valid is None else _cu(valid, np.uint8)
    a = (weights, dt, c["cam"], _cu(target))
    loss = f.flow_loss(*a, valid=v, kind=kind, huber_delta=delta, **kw)
    assert loss.dim() == 0
    flow2d, n = f.last_flow2d, int(f.last_flow_n)
    gw, = torch.autograd.grad(loss, [weights])               # weights is the only input asked for: the render's backward does not run
    # the net's gradient of the flow term alone: with weight_grad off nothing flows through the weights into the render (whose backward would add
    # ITS gradient of weight_net); the same render serves both calls - its workspace is read, never written
    loss_n = f.flow_loss(*a, valid=v, kind=kind, huber_delta=delta, weight_grad=False, **kw)
    assert torch.equal(loss_n, loss) and torch.equal(f.last_flow2d, flow2d)
    grads = (gw,) + torch.autograd.grad(loss_n, list(_wparams(f)), allow_unused=True)
    res = dict(weights=weights.detach().cpu().numpy(), flow2d=flow2d.cpu().numpy(), loss=float(loss.detach()), n=n,
               g_weights=gw.cpu().numpy(), loss_dev=loss.detach().clone(), flow2d_dev=flow2d.clone(), gw_dev=gw)
    for k, p, gr in zip(fl64.NET_NAMES, _wparams(f), grads[1:]):
        res[k] = (torch.zeros_like(p) if gr is None else gr).cpu().numpy()
    return res


def _yard(c, dev, o, d, jit, dt, target, valid=None, kind="l2", delta=1.0, mask=None, want32=True):
    a = (c["field"], o, d, T, dt, dev["weights"], jit, c["cam"], target)
    kw = dict(valid=valid, kind=kind, delta=delta, mask=mask, device="cuda")
    y64 = fl64.flowloss64(*a, **kw)
    y32 = fl64.flowloss64(*a, dtype=torch.float32, **kw) if want32 else None
    return y64, y32


def _bounds(y32, y64):
    fl = [max(v, fl64.ULP32) for v in fl64.floors(y32, y64)]
    return fl, [max(3 * v, B_FLOOR) for v in fl]


def _check(dev, y64, y32, label):
    """flow2d, loss, g_weights and the 12 net gradients of the device against the yardstick; returns (worst error / bound, the bounds)"""
    floor, bound = _bounds(y32, y64)
    worst = 0.0
    assert dev["n"] == y64["n"], (label, dev["n"], y64["n"])
    e = abs(dev["loss"] - y64["loss"]) / abs(y64["loss"]) if y64["loss"] != 0 else abs(dev["loss"])
    print(f"[flowloss] {label}: M={y64['M']} n={y64['n']} loss {y64['loss']:.6g}: error {e:.2e}, error / bound {e / bound[1]:.2f}, error / floor {e / floor[1]:.1f}")
    assert e <= bound[1], (label, "loss", e, bound[1])
    worst = max(worst, e / bound[1])
    for k in ("flow2d", "g_weights") + tuple(fl64.NET_NAMES):
        i = 0 if k == "flow2d" else 2 if k == "g_weights" else 3
        ref = y64[k]
        if np.abs(ref).max() == 0:
            assert not dev[k].any(), (label, k, "the yardstick is exactly zero")
            continue
        e = f64.rel_err(dev[k], ref)
        print(f"[flowloss] {label}: {k}: max |.| {np.abs(ref).max():.3g}, error {e:.2e}, error / bound {e / bound[i]:.2f}, error / floor {e / floor[i]:.1f}")
        assert_grad(dev[k], ref, bound[i], f"{label}:{k}")
        worst = max(worst, e / bound[i])
    zero = ~y64["mask"].any(1)
    assert not dev["flow2d"][zero].any() and not dev["g_weights"][zero].any(), (label, "a ray without masked samples must be exactly zero")
    assert not dev["g_weights"][~y64["mask"]].any(), (label, "g_weights is zero outside the masked list")
    return worst, bound


def _dt(c, steps):
    return {0: 0.0, 1: c["ts"] / 4, 3: -1.3 * c["ts"]}[steps]


# ---------------------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("R", SHAPES)
@pytest.mark.parametrize("kind", "AB")
def test_shapes(ctx, kind, R, steps):
    c = ctx[kind]
    o, d, jit, target, valid = _case(c, kind, R)
    dt = _dt(c, steps)
    dev = _device(c, o, d, jit, dt, target, valid)
    y64, y32 = _yard(c, dev, o, d, jit, dt, target, valid)
    assert len(y64["steps"]) == steps and not y64["edge"].any() and not y32["edge"].any()
    counts = y64["mask"].sum(1)
    if R >= 2:
        assert counts[-1] == 0
    if R >= 7:
        assert counts[0] == 1 and y64["n"] == R - 2
    _check(dev, y64, y32, f"{kind}:R={R}:{steps} step(s)")
    if (R, steps) == (SHAPES[0], 1):
        # the smallest case once more with descriptor bit 3: nvfi_flow_loss_fwd on the fp32 MFMA integrator (k_rk2_fwd<false>, the kernel
        # tests/test_gpu_point64.py drives through nvfi_integrate_pos) - the same rays, the same render, the same yardstick, the same bound
        f = c["f"]
        old = f.vel_fp16
        f.vel_fp16 = "fp32"
        try:
            dev8 = _device(c, o, d, jit, dt, target, valid)
        finally:
            f.vel_fp16 = old
        assert np.array_equal(dev8["weights"], dev["weights"])       # (bit 3 has no say in a training render)
        _check(dev8, y64, y32, f"{kind}:R={R}:{steps} step(s):fp32-integrator")


@pytest.mark.parametrize("kind", "AB")
def test_huber(ctx, kind):
    c = ctx[kind]
    o, d, jit, target, valid = _case(c, kind, 65)
    dt = _dt(c, 1)
    dev = _device(c, o, d, jit, dt, target, valid, kind="huber", delta=0.7)
    y64, y32 = _yard(c, dev, o, d, jit, dt, target, valid, kind="huber", delta=0.7)
    e = y64["flow2d"] - np.where(np.isfinite(target), target, 0)
    assert (np.abs(e) > 0.7).any() and (np.abs(e) < 0.7).any()          # both branches of the element are taken
    _check(dev, y64, y32, f"{kind}:huber")


# ---------------------------------------------------------------------------------------------------------------- 2. sensitivity
@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("kind", "AB")
def test_yardstick_sees_a_lost_entry(ctx, kind, steps):
    c = ctx[kind]
    dt = _dt(c, steps)
    for R in (7, 6, 5, 4):                                   # the first of these cases whose list is no multiple of the 32-entry tile
        o, d, jit, target, valid = _case(c, kind, R)
        dev = _device(c, o, d, jit, dt, target, valid)
        y64, y32 = _yard(c, dev, o, d, jit, dt, target, valid)
        if y64["M"] % 32 != 0:
            break
    assert y64["M"] % 32 != 0
    cut_mask = y64["mask"].copy()
    r, j = y64["idx"][-1]
    cut_mask[r, j] = False
    cut, _ = _yard(c, dev, o, d, jit, dt, target, valid, mask=cut_mask, want32=False)
    bound = _bounds(y32, y64)[1][3]
    s = {k: f64.rel_err(cut[k], y64[k]) for k in fl64.NET_NAMES}
    print(f"[flowloss] sensitivity {kind}, {steps} step(s), last of {y64['M']} entries: moves the net tensors by {min(s.values()):.2e} .. {max(s.values()):.2e} (bound {bound:.1e})")
    if (kind, steps) in BLIND:
        assert not any(v > bound for v in s.values()), (kind, steps, "is listed as blind but is not", s)
    else:
        assert any(v > bound for v in s.values()), (kind, steps, s)


# ---------------------------------------------------------------------------------------------------------------- 3. exact values
@pytest.mark.parametrize("kind", "AB")
def test_zero_dt_is_exact(ctx, kind):
    c = ctx[kind]
    o, d, jit, target, valid = _case(c, kind, 65)
    dev = _device(c, o, d, jit, 0.0, target, valid)
    assert not dev["flow2d"].any() and not dev["g_weights"].any() and all(not dev[k].any() for k in fl64.NET_NAMES)
    t = np.where(np.isfinite(target), target, 0)[(valid != 0) & np.isfinite(target).all(1)].astype(np.float64)
    assert dev["n"] == len(t) and abs(dev["loss"] - (t * t).sum() / (2 * len(t))) <= 1e-6 * (t * t).sum() / (2 * len(t))


@pytest.mark.parametrize("why", ("valid", "nan"))
def test_no_valid_ray_is_exact(ctx, why):
    c = ctx["A"]
    o, d, jit, target, valid = _case(c, "A", 65)
    if why == "valid":
        valid[:] = 0
    else:
        target[:, 1] = np.inf
        valid = None
    dev = _device(c, o, d, jit, _dt(c, 1), target, valid)
    assert dev["n"] == 0 and dev["loss"] == 0.0
    assert dev["flow2d"].any()                                        # the map itself does not depend on the target
    assert not dev["g_weights"].any() and all(not dev[k].any() for k in fl64.NET_NAMES)


# ---------------------------------------------------------------------------------------------------------------- 4. bit identity
def test_training_map_is_render_flows_formula(ctx):
    """with a jitter of zero the training render's samples are the eval render's: the training call's flow2d against flow64 - the yardstick of
    nvfi_render_flow - on the same weights"""
    c = ctx["A"]
    o, d, _, target, _ = _case(c, "A", 64)
    dt = _dt(c, 1)
    dev = _device(c, o, d, np.zeros(64, np.float32), dt, target)
    y = f64.flow64(c["field"], o, d, T, dt, dev["weights"], c["cam"], want=("flow2d",))
    y32 = f64.flow64(c["field"], o, d, T, dt, dev["weights"], c["cam"], dtype=torch.float32, want=("flow2d",))
    bound = max(3 * max(f64.rel_err(y32["flow2d"], y["flow2d"]), fl64.ULP32), B_FLOOR)
    e = f64.rel_err(dev["flow2d"], y["flow2d"])
    print(f"[flowloss] training map against flow64: error {e:.2e}, bound {bound:.1e}")
    assert y["M"] > 0 and e <= bound


def test_repeat(ctx):
    c = ctx["B"]
    o, d, jit, target, valid = _case(c, "B", 65)
    a = _device(c, o, d, jit, _dt(c, 3), target, valid)
    b = _device(c, o, d, jit, _dt(c, 3), target, valid)
    assert torch.equal(a["flow2d_dev"], b["flow2d_dev"]) and torch.equal(a["loss_dev"], b["loss_dev"]) and torch.equal(a["gw_dev"], b["gw_dev"])
    same = {k: bool(np.array_equal(a[k], b[k])) for k in fl64.NET_NAMES}
    print(f"[flowloss] repeat: net gradients identical: {same}")
    assert all(same.values()), same


def test_chunks(ctx):
    from nvfi_amd.utils.flow_loss import flow_loss_plan
    c = ctx["A"]
    f = c["f"]
    o, d, jit, target, valid = _case(c, "A", 64)
    dt = _dt(c, 3)
    one = _device(c, o, d, jit, dt, target, valid)
    assert f.last_flow_chunks == 1
    desc = f._desc()
    cap = 64 * desc.n_samples
    nb = C.c_int64(0)
    from nvfi_amd import _lib
    _lib.check(_lib.lib().nvfi_flow_loss_workspace_bytes(C.byref(desc), C.c_int64(64), C.c_float(T), C.c_float(dt), C.c_int64(1280), C.byref(nb)))
    many = _device(c, o, d, jit, dt, target, valid, max_workspace_bytes=nb.value + 4096)
    M = int((one["weights"] > np.float32(c["field"].thres)).sum())
    assert f.last_flow_chunks == (cap + 1279) // 1280 >= 3 and f.last_flow_workspace_bytes <= nb.value + 4096
    assert 1280 < M <= 2 * 1280, (M, "two chunks with entries, the trailing one empty")
    assert flow_loss_plan(desc, 64, T, dt, nb.value + 4096)[0] == 1280
    assert torch.equal(one["gw_dev"], many["gw_dev"]) and torch.equal(one["flow2d_dev"], many["flow2d_dev"]) and torch.equal(one["loss_dev"], many["loss_dev"])
    y64, y32 = _yard(c, one, o, d, jit, dt, target, valid)
    _check(one, y64, y32, "A:one chunk")
    _check(many, y64, y32, f"A:{f.last_flow_chunks} chunks")
    with pytest.raises(_lib.NvfiError):
        _device(c, o, d, jit, dt, target, valid, max_workspace_bytes=1 << 20)


def test_add_gw_composes_with_the_distortion_scratch(ctx):
    from nvfi_amd.utils.flow_loss import flow_loss_raw
    from nvfi_amd.utils.ray_regs import distortion_loss_raw
    c = ctx["A"]
    f = c["f"]
    o, d, jit, target, valid = _case(c, "A", 65)
    out = _render(c, o, d, jit)
    node = out[3].grad_fn
    ro, rd, w = node.saved_tensors[:3]
    desc = f._desc()
    g_dist = distortion_loss_raw(w, f.distortion_delta(), grad_scale=0.3)[1]
    a = (desc, node.ws, node.flags, ro, rd, w, T, _dt(c, 1), c["cam"], _cu(target))
    ws_before = node.ws.clone()
    sep = flow_loss_raw(*a, valid=_cu(valid, np.uint8), grad_scale=0.7)
    both = g_dist.clone()
    add = flow_loss_raw(*a, valid=_cu(valid, np.uint8), grad_scale=0.7, g_weights=both, add_gw=True)
    assert add["g_weights"] is both and torch.equal(both, g_dist + sep["g_weights"])
    assert sep["g_weights"].any() and torch.equal(add["loss"], sep["loss"]) and torch.equal(add["flow2d"], sep["flow2d"])
    assert torch.equal(node.ws, ws_before), "the render workspace is read, never written"


def _is_weight_net(name):
    return "vel_net.weight_net" in name


_det = {}


def _det_child(tmp_path_factory):
    """tests/flowloss_det_check.py in a child process with NVFI_DETERMINISTIC=1 (read once per process: the plane scatter and the weight-gradient
    reduce then repeat bit for bit), once for the two tests that need it -> (its JSON line, its .npz)"""
    if not _det:
        import json
        import subprocess
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = str(tmp_path_factory.mktemp("flowloss_det") / "grads.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "flowloss_det_check.py"), path], env=dict(os.environ, NVFI_DETERMINISTIC="1"),
                           cwd=root, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        _det["json"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        _det["npz"] = dict(np.load(path))
    return _det["json"], _det["npz"]


def test_render_gradients_are_untouched(tmp_path_factory):
    """the flow term with weight_grad off leaves the render's own share of the backward alone: the workspace has the same bytes before and after
    the call, and EVERY parameter outside weight_net gets the gradient of the plain render bit for bit.  Run with NVFI_DETERMINISTIC=1 in a child
    process, where two plain backwards repeat bit for bit (the default plane scatter adds in an order that differs from run to run)."""
    res, _ = _det_child(tmp_path_factory)
    bad = [k for k, v in res["plain_repeats"].items() if not v]
    assert not bad, ("two plain runs differ: the deterministic mode is not on", bad)
    assert res["ws_same"], "the render workspace is read, never written"
    bad = [k for k, v in res["untouched"].items() if not v]
    print(f"[flowloss] render gradients with the flow term (weight_grad off): {len(res['untouched']) - len(bad)} of {len(res['untouched'])} tensors bit-identical")
    assert not bad and res["none_stay_none"], bad
    assert len(res["untouched"]) >= 7
    assert len(res["net_moved"]) == 12 and all(res["net_moved"].values()), ("the flow term reaches weight_net", res["net_moved"])


def _fused(c, o, d, jit, rgb_t, **kw):
    model, f = c["model"], c["f"]
    model.zero_grad(set_to_none=True)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    model.train()
    return f.render_mse_backward_(T, _cu(o), _cu(d), rgb_t, white_bg=True, jitter=_cu(jit), **kw)


def test_fused_and_autograd_forms_agree(ctx, tmp_path_factory):
    """the gradients of SCALE * (mse + LAM * flow_loss) through autograd and of the fused driver, formed in the deterministic child process.  The 12
    weight_net tensors - what the flow term reaches directly - through assert_grad under the yardstick's bound for the net gradients of this case,
    max(3 x floor, 1e-5).  The render's own tensors, for which the yardstick has no floor, through assert_grad under 1e-5, the bound with its floor
    at one fp32 ulp (3 x 1.2e-7 < 1e-5): the two forms hand the same launches the same g_weights bits (SCALE and LAM are powers of two) and differ
    only in the rounding of the colour gradient."""
    c = ctx["A"]
    model, f = c["model"], c["f"]
    o, d, jit, target, valid = _case(c, "A", 65)
    dt = _dt(c, 1)
    _, z = _det_child(tmp_path_factory)
    assert abs(z["flow"][0] - z["flow"][1]) == 0.0, "the same forward call: the same value"
    y64, y32 = _yard(c, dict(weights=z["weights"]), o, d, jit, dt, target, valid)
    floor, bound = _bounds(y32, y64)
    names = [k[4:] for k in z if k.startswith("ref:")]
    net = [k for k in names if _is_weight_net(k)]
    assert len(net) == 12 and len(names) >= 19
    for k in names:
        b = bound[3] if _is_weight_net(k) else B_FLOOR
        e = f64.rel_err(z["got:" + k], z["ref:" + k])
        same = np.array_equal(z["got:" + k], z["ref:" + k])
        print(f"[flowloss] fused against autograd: {k}: error {e:.2e}, error / bound {e / b:.2f}{', bit-identical' if same else ''}")
    for k in names:
        assert_grad(z["got:" + k], z["ref:" + k], bound[3] if _is_weight_net(k) else B_FLOOR, f"fused:{k}")
    # the shape of the fused call's result, in this process
    rgb_t = _cu(np.random.default_rng(3).random((65, 3)))
    LAM, SCALE = 0.5, 0.25
    out = _render(c, o, d, jit)
    flow = f.flow_loss(out[3], dt, c["cam"], _cu(target), valid=_cu(valid, np.uint8)).detach()
    del out
    cam_dev = (_cu(c["cam"][0]),) + tuple(c["cam"][1:])
    res = _fused(c, o, d, jit, rgb_t, loss_scale=SCALE, target_flow=_cu(target), flow_dt=dt, flow_camera=cam_dev, flow_weight=LAM, flow_valid=_cu(valid, np.uint8))
    assert len(res) == 3 and res[2].dim() == 0 and torch.equal(res[2], flow)
    # without the keyword: the two-tuple; with the distortion term: (loss, rgb, distortion, flow), the flow value unchanged
    assert len(_fused(c, o, d, jit, rgb_t)) == 2
    res4 = _fused(c, o, d, jit, rgb_t, distortion_weight=0.1, target_flow=_cu(target), flow_dt=dt, flow_camera=cam_dev, flow_valid=_cu(valid, np.uint8))
    assert len(res4) == 4 and torch.equal(res4[3], res[2])
    from nvfi_amd.models.tensorf_keyframe import DeviceTime
    with pytest.raises(NotImplementedError):
        f.render_mse_backward_(DeviceTime(T, torch.tensor([T], device="cuda")), _cu(o), _cu(d), rgb_t, jitter=_cu(jit), target_flow=_cu(target), flow_dt=dt,
                               flow_camera=cam_dev)
    model.zero_grad(set_to_none=True)


def test_graph_replay_of_the_fused_step(ctx):
    c = ctx["A"]
    model, f = c["model"], c["f"]
    o, d, jit, target, valid = _case(c, "A", 65)
    dt = _dt(c, 1)
    rgb_t = _cu(np.random.default_rng(3).random((65, 3)))
    cam_dev = (_cu(c["cam"][0]),) + tuple(c["cam"][1:])
    ot, dtt, jt, tt, vt = _cu(o), _cu(d), _cu(jit), _cu(target), _cu(valid, np.uint8)
    kw = dict(white_bg=True, jitter=jt, target_flow=tt, flow_dt=dt, flow_camera=cam_dev, flow_weight=0.5, flow_valid=vt)
    model.zero_grad(set_to_none=True)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    model.train()
    eager = [x.clone() for x in f.render_mse_backward_(T, ot, dtt, rgb_t, **kw)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        out = f.render_mse_backward_(T, ot, dtt, rgb_t, **kw)
    torch.cuda.current_stream().wait_stream(cap)
    for x in out:
        x.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 3
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals on the device
def test_refusals(ctx):
    from nvfi_amd import _lib
    c = ctx["A"]
    f = c["f"]
    o, d, jit, target, valid = _case(c, "A", 7)
    out = _render(c, o, d, jit)
    tg = _cu(target)
    with pytest.raises(ValueError):
        f.flow_loss(out[3].detach(), 0.1, c["cam"], tg)                       # not the render's own tensor
    with pytest.raises(ValueError):
        f.flow_loss(torch.rand(7, out[3].shape[1], device="cuda", requires_grad=True) * 1.0, 0.1, c["cam"], tg)
    with pytest.raises(ValueError):
        ctx["B"]["f"].flow_loss(out[3], 0.1, c["cam"], tg)                    # another field's render
    with pytest.raises(_lib.NvfiError, match="error 2"):
        f.flow_loss(out[3], 32.25 * c["ts"], c["cam"], tg)                    # 65 steps: refused, not truncated
    with pytest.raises(ValueError):
        f.flow_loss(out[3], 0.1, c["cam"], tg, kind="l1")
    twice = f.flow_loss(out[3], 0.1, c["cam"], tg, weight_grad=False)         # (the render's backward does not run: its workspace stays)
    twice.backward(retain_graph=True)
    with pytest.raises(ValueError, match="released"):
        twice.backward()                                                      # the first backward released the call's workspace
    from nvfi_amd.models import MaskField
    f.mask_field = MaskField(n_layer=4, n_dim=128, skips=[], mask_dim=8).cuda()
    try:
        masked = _render(c, o, d, jit)
        with pytest.raises(NotImplementedError):
            f.flow_loss(masked[3], 0.1, c["cam"], tg)                         # a render of the mask branch
        del masked
    finally:
        f.mask_field = None
    loss = f.flow_loss(out[3], 0.1, c["cam"], tg)
    (out[0].sum() + loss).backward()
    with pytest.raises(ValueError, match="released"):
        f.flow_loss(out[3], 0.1, c["cam"], tg)                                # the backward has freed the workspace
    c["model"].eval()
    with torch.no_grad():
        ev = f(T, _cu(o), _cu(d), True)
    with pytest.raises(ValueError):
        f.flow_loss(ev[3], 0.1, c["cam"], tg)                                 # an eval render
    c["model"].zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------------------------- 6. evaluation
def test_evaluation_reports_the_end_point_error(ctx):
    from nvfi_amd.models import Camera, Renderer
    from nvfi_amd.utils import render_test_evaluation
    c = ctx["A"]
    model, f = c["model"], c["f"]
    H = W = 24
    focal = c["cam"][3] * H / c["cam"][1]
    pose = torch.eye(4)
    pose[:3, :4] = torch.from_numpy(np.asarray(c["cam"][0]))
    near, far = [float(v) for v in f.near_far]
    dt = c["ts"] / 4
    rng = np.random.default_rng(9)
    gt = rng.standard_normal((H, W, 2)).astype(np.float32)
    gt[0, 0, 0] = np.nan
    ok = rng.random((H, W)) < 0.8
    ren = Renderer(model, 0, 0, 2048)
    res = render_test_evaluation(model, ren, [pose.numpy()], [T], None, H, W, focal, near, far, update_alpha_mask=False, gt_flows=[gt], flow_dt=dt,
                                 flow_valid=[ok])
    assert len(res["epe"]) == 1 and res["mean_epe"] == res["epe"][0] and res["flow2d"].shape == (1, H, W, 2)
    model.eval()
    cam = Camera(pose.cuda(), H, W, focal, None, near, far)
    rays = cam.rays
    with torch.no_grad():
        w = ren.render(T, rays.to("cuda"), white_background=True, mode="test")[3].reshape(H * W, -1).cpu().numpy()
    ro, rd = rays.ray_origins.reshape(-1, 3).cpu().numpy(), rays.ray_directions.reshape(-1, 3).cpu().numpy()
    camt = (c["cam"][0], H, W, focal)
    y = f64.flow64(c["field"], ro, rd, T, dt, w, camt, want=("flow2d",))
    y32 = f64.flow64(c["field"], ro, rd, T, dt, w, camt, dtype=torch.float32, want=("flow2d",))
    ref = fl64.epe(y["flow2d"], gt, ok)
    tol = max(3 * max(f64.rel_err(y32["flow2d"], y["flow2d"]), fl64.ULP32), B_FLOOR) * max(np.abs(y["flow2d"]).max(), 1.0)
    print(f"[flowloss] EPE {res['epe'][0]:.6g}, yardstick {ref:.6g}, tolerance {tol:.1e}")
    assert abs(res["epe"][0] - ref) <= tol + 1e-6 * ref
    plain = render_test_evaluation(model, ren, [pose.numpy()], [T], None, H, W, focal, near, far, update_alpha_mask=False)
    assert "epe" not in plain
    with pytest.raises(ValueError):
        render_test_evaluation(model, ren, [pose.numpy()], [T], None, H, W, focal, near, far, update_alpha_mask=False, gt_flows=[gt])
