"""2-D mask supervision on the device - field.mask_loss, field.mask_fit_backward_, render_mse_backward_(target_mask=) (nvfi_mask_loss_fwd /
nvfi_mask_loss_bwd; csrc/maskloss.hip) - against the float64 yardstick tests/maskloss64.py on the device's OWN weights and list.

Bound per tensor (mask_map, g_weights and the ten MaskField gradients relative to the tensor's max, the loss as a relative error):
maskloss64.bounds = max(3 x the case's own float32 distance, the floor of maskloss64.py).  The float32 distance is maskloss64(float32) against
maskloss64(float64) on the same inputs, measured in the test; nothing is derived from the device.  Every comparison prints error / bound.

Rays (maskloss64.gpu_rays): the golden rays of the hot-path fixture, rendered in training mode with a per-ray jitter from the seed table of
maskloss64.py; from R = 2 on a case ends in a ray that looks away from the box (no masked sample: exact zeros), and from R = 33 on it carries one
background ray, one ignored ray (label -1 / a NaN row).
MaskFields: maskfield64.params_for(K), K = 2, 8, 17, 32 (the trunk of tests/golden/maskfield.npz; from K = 9 on accumulator registers 4..15 of the
logit tile carry live rows, from K = 17 on both half-waves hold rows >= 8).

ReLU kinks: the render's points cannot be redrawn.  Every matrix case computes maskfield64.margin on the yardstick's positions, asserts that the
share of entries with margin < 1 is <= maskfield64.KINK_CAP, and admits the flips the device took (maskfield64.admit_flips) before comparing the
ten gradients under the UNCHANGED bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import maskfield64 as m64
import maskloss64 as ml64
import render64 as r64
from helpers import field_state, make_model

pytestmark = pytest.mark.gpu

T = 19.0 / 60.0
SHAPES = (1, 2, 33, 257)
KS = (2, 8, 17, 32)
EPS = 1e-5


def _cu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _mask_field(K):
    from nvfi_amd.models import MaskField
    mf = MaskField(n_layer=4, n_dim=128, input_dim=3, skips=[], mask_dim=K, mask_act="softmax")
    with torch.no_grad():
        for p, v in zip(mf._params(), m64.params_for(K)):
            p.copy_(torch.from_numpy(v))
    return mf.cuda()


def _make_ctx(gold, kinds="AB"):
    out = {}
    mfs = {K: _mask_field(K) for K in KS}
    for kind in kinds:
        model, meta = make_model(kind)
        out[kind] = dict(model=model, f=model.nvfi, field=r64.Field(*field_state(model)), gold=gold, kind=kind, mfs=mfs)
    return out


@pytest.fixture(scope="module")
def ctx(gold):
    out = _make_ctx(gold)
    yield out
    for c in out.values():
        c["f"].mask_field = None


def _render(c, o, d, jit, t=T):
    """one TRAINING render with the given per-ray jitter -> the field's outputs (weights carries the autograd node)"""
    f = c["f"]
    f.mask_field = None
    c["model"].train()
    f.jitter_override = torch.from_numpy(np.ascontiguousarray(jit, dtype=np.float32)).reshape(-1, 1)
    try:
        return f(t, _cu(o), _cu(d), True)
    finally:
        f.jitter_override = None


def _rays(c, R):
    """maskloss64.gpu_rays: the rays and the jitter whose kink share tests/test_maskloss_golden.py checks on the CPU"""
    return ml64.gpu_rays(c["gold"], c["kind"], R)


def _target(R, K, soft, seed=0):
    """labels (int32) or soft rows (float32) of a case; from R = 33 on ray 1 is background and ray 2 is ignored"""
    rng = np.random.default_rng(5 + R + 100 * K + seed)
    if not soft:
        lab = rng.integers(0, K, R).astype(np.int32)
        if R >= 33:
            lab[1], lab[2] = K, -1
        return lab
    y = rng.random((R, K)).astype(np.float32)
    y = y / y.sum(1, keepdims=True) * rng.random((R, 1)).astype(np.float32)      # rows that sum to an opacity in [0, 1)
    if R >= 33:
        y[1] = 0.0
        y[2, K - 1] = np.nan
    return y.astype(np.float32)


def _device(c, K, o, d, jit, target, kind="ce", **kw):
    """value and gradients on the device: dict(mask_map, loss, n, g_weights, <ten names>) as numpy + device tensors under *_dev"""
    f, mf = c["f"], c["mfs"][K]
    out = _render(c, o, d, jit)
    weights = out[3]
    tg = _cu(target, np.int32 if target.dtype.kind == "i" else np.float32)
    loss = f.mask_loss(weights, tg, mask_field=mf, kind=kind, eps=EPS, **kw)
    assert loss.dim() == 0
    mask_map, n = f.last_mask_map, int(f.last_mask_n)
    grads = torch.autograd.grad(loss, [weights] + list(mf._params()), allow_unused=True)   # weights is an input asked for: the render's backward does not run
    res = dict(weights=weights.detach().cpu().numpy(), mask_map=mask_map.cpu().numpy(), loss=float(loss.detach()), n=n, g_weights=grads[0].cpu().numpy(),
               loss_dev=loss.detach().clone(), map_dev=mask_map.clone(), gw_dev=grads[0], grads_dev=grads[1:])
    for k, p, gr in zip(ml64.GRAD_KEYS, mf._params(), grads[1:]):
        res[k] = (torch.zeros_like(p) if gr is None else gr).cpu().numpy()
    return res


def _yard(c, K, dev, o, d, jit, target, kind="ce", mask=None):
    a = (c["field"], m64.params_for(K), o, d, T, dev["weights"], jit, target)
    y64 = ml64.maskloss64(*a, kind=kind, eps=EPS, mask=mask, device="cuda")
    y32 = ml64.maskloss64(*a, kind=kind, eps=EPS, mask=mask, dtype=torch.float32, want_margin=False)
    return y64, y32


def _check(dev, y64, y32, label, target=None, kind="ce", K=None):
    """mask_map, loss, n, g_weights and the ten gradients of the device against the yardstick; returns the bounds"""
    bound = ml64.bounds(y32, y64)
    assert dev["n"] == y64["n"], (label, dev["n"], y64["n"])
    e = abs(dev["loss"] - y64["loss"]) / abs(y64["loss"]) if y64["loss"] != 0 else abs(dev["loss"])
    print(f"[maskloss] {label}: M={y64['M']} n={y64['n']} loss {y64['loss']:.6g}: error {e:.2e}, error / bound {e / bound[1]:.2f}")
    assert e <= bound[1], (label, "loss", e, bound[1])
    ref = y64
    if target is not None and y64["M"]:
        mg = y64["margin"]
        share = float((mg < 1.0).mean())
        assert share <= m64.KINK_CAP, (label, "share of entries within one rounding bound of a ReLU kink", share)
        if (mg < 1.0).any():
            flips = ml64.entry_flips(m64.params_for(K), y64, target, kind, EPS)
            ref, taken = m64.admit_flips(dev, {k: y64[k] for k in ml64.GRAD_KEYS}, flips)
            ref = dict(y64, **ref)
            print(f"[maskloss] {label}: {int((mg < 1.0).sum())} entries with margin < 1, {len(flips)} listed gates, admitted {taken}")
    for k in ("mask_map", "g_weights") + tuple(ml64.GRAD_KEYS):
        i = 0 if k == "mask_map" else 2 if k == "g_weights" else 3
        if np.abs(ref[k]).max() == 0:
            assert not dev[k].any(), (label, k, "the yardstick is exactly zero")
            continue
        e = ml64.rel_err(dev[k], ref[k])
        print(f"[maskloss] {label}: {k}: max |.| {np.abs(ref[k]).max():.3g}, error {e:.2e}, error / bound {e / bound[i]:.2f}")
        assert e <= bound[i], (label, k, e, bound[i])
    zero = ~y64["mask"].any(1)
    assert not dev["mask_map"][zero].any() and not dev["g_weights"][zero].any(), (label, "a ray without masked samples must be exactly zero")
    assert not dev["g_weights"][~y64["mask"]].any(), (label, "g_weights is zero outside the masked list")
    assert not dev["g_weights"][~y64["ok"]].any(), (label, "an ignored ray has no gradient")
    return bound


# ---------------------------------------------------------------------------------------------------------------- 1. value and gradient matrix
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", SHAPES)
@pytest.mark.parametrize("kind", "AB")
def test_matrix(ctx, kind, R, K):
    """both loss kinds, labels and soft rows, on one render of the case"""
    c = ctx[kind]
    o, d, jit = _rays(c, R)
    for lk in ("ce", "l2"):
        for soft in (False, True):
            target = _target(R, K, soft)
            dev = _device(c, K, o, d, jit, target, lk)
            y64, y32 = _yard(c, K, dev, o, d, jit, target, lk)
            counts = y64["mask"].sum(1)
            if R >= 2:
                assert counts[-1] == 0
            if R >= 33:
                assert y64["n"] == R - 1
            if R >= 257:
                assert y64["M"] > 128                                # more than one workgroup of entries
            _check(dev, y64, y32, f"{kind}:R={R}:K={K}:{lk}:{'soft' if soft else 'labels'}", target, lk, K)


@pytest.mark.parametrize("kind", "AB")
def test_yardstick_sees_a_lost_entry_and_a_swapped_label(ctx, kind):
    """what the bound would catch: the yardstick with the LAST masked entry dropped, and with two labels swapped, leaves the device's result"""
    c = ctx[kind]
    K, R = 8, 33
    o, d, jit = _rays(c, R)
    target = _target(R, K, False)
    dev = _device(c, K, o, d, jit, target, "ce")
    y64, y32 = _yard(c, K, dev, o, d, jit, target, "ce")
    bound = ml64.bounds(y32, y64)
    cut = y64["mask"].copy()
    r, s = y64["idx"][-1]
    cut[r, s] = False
    ycut, _ = _yard(c, K, dev, o, d, jit, target, "ce", mask=cut)
    moved = max(ml64.rel_err(dev[k], ycut[k]) for k in ml64.GRAD_KEYS)
    assert moved > bound[3], (moved, bound)
    sw = target.copy()
    a, b = [i for i in range(R) if 0 <= target[i] < K and y64["mask"][i].any()][:2]
    if sw[a] == sw[b]:
        sw[b] = (sw[b] + 1) % K
    sw[a], sw[b] = sw[b], sw[a]
    ysw, _ = _yard(c, K, dev, o, d, jit, sw, "ce")
    assert abs(dev["loss"] - ysw["loss"]) / abs(ysw["loss"]) > bound[1] and ml64.rel_err(dev["g_weights"], ysw["g_weights"]) > bound[2]


# ---------------------------------------------------------------------------------------------------------------- 2. bits
def _zero_grads(mf):
    for p in mf._params():
        p.grad = torch.zeros_like(p)


@pytest.mark.parametrize("kind,K", (("A", 8), ("B", 17)))
def test_mask_map_has_the_bits_of_render_mask(ctx, kind, K):
    """an eval render with the MaskField attached (nvfi_render_mask) and mask_fit_backward_ on the same rays: the same mask map, bit for bit"""
    c = ctx[kind]
    f, mf = c["f"], c["mfs"][K]
    o, d, _ = _rays(c, 257)
    c["model"].eval()
    f.mask_field = mf
    try:
        with torch.no_grad():
            ref = f(T, _cu(o), _cu(d), True)[4]
    finally:
        f.mask_field = None
    _zero_grads(mf)
    tg = _cu(_target(257, K, False), np.int32)
    loss, mm = f.mask_fit_backward_(T, _cu(o), _cu(d), tg, mask_field=mf)
    assert ref.shape == mm.shape == (257, K) and ref.any() and torch.equal(ref, mm) and f.last_mask_chunks == 1
    g1 = [p.grad.clone() for p in mf._params()]
    # a smaller plan in a workspace the caller keeps: more chunks, the same value and map bits, the same gradients to the chunking's rounding
    from nvfi_amd.models.mask_field import _mask_desc
    from nvfi_amd.utils.mask_loss import mask_loss_plan
    small = 120 << 20
    plan = mask_loss_plan(f._desc(), _mask_desc(mf, mf._params()), 257, small)
    ws = torch.empty(plan[1], dtype=torch.uint8, device="cuda")
    _zero_grads(mf)
    loss2, mm2 = f.mask_fit_backward_(T, _cu(o), _cu(d), tg, mask_field=mf, max_workspace_bytes=small, workspace=ws)
    assert f.last_mask_chunks == plan[2] > 1 and f.last_mask_workspace_bytes == plan[1] <= small
    assert torch.equal(loss2, loss) and torch.equal(mm2, mm)
    for a, b in zip(g1, (p.grad for p in mf._params())):
        assert ml64.rel_err(b.cpu().numpy(), a.cpu().numpy()) <= ml64.FLOOR_G
    with pytest.raises(ValueError):
        f.mask_fit_backward_(T, _cu(o), _cu(d), tg, mask_field=mf, max_workspace_bytes=small, workspace=ws[:-1])
    mf.zero_grad(set_to_none=True)


def test_repeat(ctx):
    c = ctx["B"]
    o, d, jit = _rays(c, 257)
    target = _target(257, 17, True)
    a = _device(c, 17, o, d, jit, target, "ce")
    b = _device(c, 17, o, d, jit, target, "ce")
    assert torch.equal(a["map_dev"], b["map_dev"]) and torch.equal(a["loss_dev"], b["loss_dev"]) and torch.equal(a["gw_dev"], b["gw_dev"])
    same = {k: bool(np.array_equal(a[k], b[k])) for k in ml64.GRAD_KEYS}
    print(f"[maskloss] repeat: MaskField gradients identical: {same}")
    assert all(same.values()), same


def test_chunks(ctx):
    """a chunk_cap that splits the list into three chunks, the last partly filled, and further chunks wholly beyond the count.  mask_map, loss and
    g_weights do not depend on the chunking: bit-identical.  The ten gradients: the split-K weight-gradient sums run per chunk (another
    association of the same sums, and one atomic add per chunk), so they are held to the SAME float64 bound, not to the one-chunk bits."""
    from nvfi_amd import _lib
    from nvfi_amd.utils.mask_loss import mask_loss_plan
    c = ctx["A"]
    f, K, R = c["f"], 8, 65
    o, d, jit = _rays(c, R)
    target = _target(R, K, False)
    one = _device(c, K, o, d, jit, target, "ce")
    assert f.last_mask_chunks == 1
    M = int((one["weights"] > np.float32(c["field"].thres)).sum())
    desc = f._desc()
    cap = R * desc.n_samples
    chunk = next(128 * k for k in range(1, 64) if -(-M // (128 * k)) == 3 and M % (128 * k))
    from nvfi_amd.models.mask_field import _mask_desc
    md = _mask_desc(c["mfs"][K], c["mfs"][K]._params())
    nb = _lib.bytes_of(_lib.lib().nvfi_mask_loss_workspace_bytes, C.byref(desc), C.byref(md), C.c_int64(R), C.c_int64(chunk))
    many = _device(c, K, o, d, jit, target, "ce", max_workspace_bytes=nb + 4096)
    assert mask_loss_plan(desc, md, R, nb + 4096)[0] == chunk
    assert f.last_mask_chunks == -(-cap // chunk) >= 4 and f.last_mask_workspace_bytes <= nb + 4096, (f.last_mask_chunks, M, chunk, cap)
    assert torch.equal(one["gw_dev"], many["gw_dev"]) and torch.equal(one["map_dev"], many["map_dev"]) and torch.equal(one["loss_dev"], many["loss_dev"])
    y64, y32 = _yard(c, K, one, o, d, jit, target, "ce")
    _check(one, y64, y32, "A:one chunk", target, "ce", K)
    _check(many, y64, y32, f"A:{f.last_mask_chunks} chunks of {chunk} (M = {M})", target, "ce", K)
    same = {k: bool(np.array_equal(one[k], many[k])) for k in ml64.GRAD_KEYS}
    print(f"[maskloss] chunks: gradients bit-identical to the one-chunk call: {same}")
    with pytest.raises(_lib.NvfiError):
        _device(c, K, o, d, jit, target, "ce", max_workspace_bytes=1 << 20)


@pytest.mark.parametrize("why", ("no masked sample", "every ray ignored"))
def test_exact_zeros(ctx, why):
    c = ctx["A"]
    K, R = 8, 33
    o, d, jit = _rays(c, R)
    if why == "no masked sample":
        d[:-1] = -d[:-1]                 # every ray looks away from the box (_rays turned the last one already): M = 0
        target = _target(R, K, False)
    else:
        target = np.full(R, -1, np.int32)
    for lk in ("ce", "l2"):
        dev = _device(c, K, o, d, jit, target, lk)
        if why == "no masked sample":
            assert not (dev["weights"] > np.float32(c["field"].thres)).any() and dev["n"] == R - 1
            assert not dev["mask_map"].any()
            want = float((R - 2) / (2.0 * (R - 1) * K)) if lk == "l2" else float(-np.log(np.float64(np.float32(EPS))) * (R - 2) / (R - 1))
            assert abs(dev["loss"] - want) <= 4e-7 * abs(want), (lk, dev["loss"], want)      # q = 0 exactly: the loss of the targets alone
        else:
            assert dev["n"] == 0 and dev["loss"] == 0.0
        assert not dev["g_weights"].any()
        for k in ml64.GRAD_KEYS:
            assert not dev[k].any(), (why, lk, k)


def test_add_gw_composes_with_the_distortion_scratch(ctx):
    from nvfi_amd.models.mask_field import _mask_desc
    from nvfi_amd.utils.mask_loss import mask_loss_raw
    from nvfi_amd.utils.ray_regs import distortion_loss_raw
    c = ctx["A"]
    f, K, R = c["f"], 8, 33
    mf = c["mfs"][K]
    o, d, jit = _rays(c, R)
    out = _render(c, o, d, jit)
    node = out[3].grad_fn
    w = node.saved_tensors[2]
    desc, md = f._desc(), _mask_desc(mf, mf._params())
    g_dist = distortion_loss_raw(w, f.distortion_delta(), grad_scale=0.3)[1]
    a = (desc, md, node.ws, node.flags, w, T, _cu(_target(R, K, False), np.int32))
    ws_before = node.ws.clone()
    sep = mask_loss_raw(*a, grad_scale=0.7)
    both = g_dist.clone()
    add = mask_loss_raw(*a, grad_scale=0.7, g_weights=both, add_gw=True)
    assert add["g_weights"] is both and torch.equal(both, g_dist + sep["g_weights"])
    assert sep["g_weights"].any() and torch.equal(add["loss"], sep["loss"]) and torch.equal(add["mask_map"], sep["mask_map"])
    assert torch.equal(node.ws, ws_before), "the render workspace is read, never written"


# ---------------------------------------------------------------------------------------------------------------- 3. the fused forms
def _host_assembled(c, K, o, d, target, kind):
    """the form that exists without this term, on the render mask_fit_backward_ makes (eval mode): the host read of the masked count, the export
    of the masked samples, MaskField through its own autograd boundary (what _mask_map_train does behind a training render), torch composite
    and torch loss -> (loss, mask map, the ten gradients, the weights, the exported positions)"""
    from nvfi_amd import _lib
    f, mf = c["f"], c["mfs"][K]
    c["model"].eval()
    f.mask_field = mf
    try:
        with torch.no_grad():
            w = f(T, _cu(o), _cu(d), True)[3]
        R, S = w.shape
        M = int(f.last_counters[2])
        xyz = torch.empty(M, 3, device="cuda")
        idx = torch.empty(M, dtype=torch.int64, device="cuda")
        Rl, t, flags = f._last_call
        desc = f._desc()
        _lib.check(_lib.lib().nvfi_render_export_masked(C.byref(desc), C.c_int64(R), C.c_float(t), C.c_int(flags), _lib.ptr(f._last_ws),
                                                        C.c_int64(f._last_ws.numel()), C.c_int64(M), _lib.ptr(xyz), _lib.ptr(idx), None))
    finally:
        f.mask_field = None
    torch.cuda.synchronize()
    mf.zero_grad(set_to_none=True)
    m = mf(xyz)
    q = torch.zeros(R, K, device="cuda").index_add(0, idx // S, w.reshape(-1)[idx][:, None] * m)
    y, ok = ml64.targets(target, R, K)
    y, okt = _cu(y), torch.from_numpy(ok).cuda()
    n = int(ok.sum())
    if kind == "l2":
        loss = (((q - y) ** 2) * okt[:, None]).sum() / (2 * n * K)
    else:
        loss = (torch.where(y != 0, -y * torch.log(q + EPS), torch.zeros_like(q)) * okt[:, None]).sum() / n
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in zip(ml64.GRAD_KEYS, mf._params())}
    mf.zero_grad(set_to_none=True)
    return float(loss.detach()), q.detach().cpu().numpy(), grads, w.cpu().numpy(), xyz.cpu().numpy()


@pytest.mark.parametrize("lk", ("ce", "l2"))
def test_mask_fit_agrees_with_the_host_assembled_path(ctx, lk):
    """mask_fit_backward_ against the host-assembled path within the SAME bounds as the matrix (maskloss64.bounds on the eval render's weights), and
    both against the float64 yardstick.  The host path is rebuilt here from its own export on an eval render - the steps of _mask_map_train (host
    read of the masked count, nvfi_render_export_masked, MaskField autograd, torch index_add) + a torch loss - and does not call _mask_map_train
    itself: that method sits behind a TRAINING forward (its jitter, its sampling rules), while mask_fit_backward_ renders in eval mode."""
    c = ctx["A"]
    f, K, R = c["f"], 8, 257
    mf = c["mfs"][K]
    o, d, _ = _rays(c, R)
    target = _target(R, K, False)
    hl, hq, hg, w, xyz = _host_assembled(c, K, o, d, target, lk)
    _zero_grads(mf)
    loss, mm = f.mask_fit_backward_(T, _cu(o), _cu(d), _cu(target, np.int32), mask_field=mf, kind=lk, eps=EPS)
    got = dict(loss=float(loss), mask_map=mm.cpu().numpy(), n=int(f.last_mask_n), weights=w, g_weights=np.zeros_like(w))
    for k, p in zip(ml64.GRAD_KEYS, mf._params()):
        got[k] = p.grad.detach().cpu().numpy().copy()
    mf.zero_grad(set_to_none=True)
    a = (c["field"], m64.params_for(K), o, d, T, w, None, target)
    y64 = ml64.maskloss64(*a, kind=lk, eps=EPS, device="cuda")
    y32 = ml64.maskloss64(*a, kind=lk, eps=EPS, dtype=torch.float32, want_margin=False)
    bound = ml64.bounds(y32, y64)
    # the device's positions are the ones the yardstick warps to, to fp32 rounding of the warp
    assert np.abs(xyz - y64["x"]).max() < 1e-4
    y64["g_weights"] = np.zeros_like(w)          # mask_fit_backward_ forms none
    _check(got, y64, y32, f"mask_fit:{lk}", target, lk, K)
    el, em = abs(got["loss"] - hl) / abs(hl), ml64.rel_err(got["mask_map"], hq)
    print(f"[maskloss] mask_fit against the host-assembled path: {lk}: loss {el:.2e} (bound {bound[1]:.2e}), mask_map {em:.2e} (bound {bound[0]:.2e})")
    assert el <= bound[1] and em <= bound[0], (el, em, bound)
    for k in ml64.GRAD_KEYS:
        e = ml64.rel_err(got[k], hg[k])
        print(f"[maskloss] mask_fit against the host-assembled path: {lk}: {k}: {e:.2e} (bound {bound[3]:.2e})")
        assert e <= bound[3], (k, e)


def test_graph_replay_of_mask_fit(ctx):
    c = ctx["A"]
    f, K, R = c["f"], 8, 257
    mf = c["mfs"][K]
    o, d, _ = _rays(c, R)
    ot, dt_, tg = _cu(o), _cu(d), _cu(_target(R, K, False), np.int32)
    c["model"].eval()
    _zero_grads(mf)
    eager = [x.clone() for x in f.mask_fit_backward_(T, ot, dt_, tg, mask_field=mf)]
    eager_g = [p.grad.clone() for p in mf._params()]
    torch.cuda.synchronize()
    for p in mf._params():
        p.grad.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        out = f.mask_fit_backward_(T, ot, dt_, tg, mask_field=mf)
    torch.cuda.current_stream().wait_stream(cap)
    for x in out:
        x.fill_(-7.0)
    for p in mf._params():
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    for p, g in zip(mf._params(), eager_g):
        assert torch.equal(p.grad, g)
    mf.zero_grad(set_to_none=True)


def _fused(c, K, o, d, jit, rgb_t, **kw):
    model, f, mf = c["model"], c["f"], c["mfs"][K]
    model.zero_grad(set_to_none=True)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    _zero_grads(mf)
    model.train()
    f.mask_field = None
    return f.render_mse_backward_(T, _cu(o), _cu(d), rgb_t, white_bg=True, jitter=_cu(jit), mask_field=mf, **kw)


_det = {}


def _det_child(tmp_path_factory):
    """tests/maskloss_det_check.py in a child process with NVFI_DETERMINISTIC=1 (read once per process: the plane scatter and the weight-gradient
    reduce then repeat bit for bit) -> its .npz"""
    if not _det:
        import subprocess
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = str(tmp_path_factory.mktemp("maskloss_det") / "grads.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "maskloss_det_check.py"), path], env=dict(os.environ, NVFI_DETERMINISTIC="1"),
                           cwd=root, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        _det["npz"] = dict(np.load(path))
    return _det["npz"]


def test_fused_and_autograd_forms_agree(ctx, tmp_path_factory):
    """the gradients of SCALE * (mse + LAM * mask_loss) through autograd and of the fused driver, formed in the deterministic child process.  The
    ten MaskField tensors under the yardstick's bound for this case.  The render's own tensors, for which the yardstick has no floor, BIT FOR BIT:
    the two forms hand the same launches the same g_weights bits and the same colour gradient - SCALE and LAM are powers of two, so scaling on
    the host or inside the kernels rounds alike - and under NVFI_DETERMINISTIC=1 the plane scatter and the weight-gradient reduce add in a
    fixed order."""
    c = ctx["A"]
    K, R = 8, 33
    o, d, jit = _rays(c, R)
    target = _target(R, K, False)
    z = _det_child(tmp_path_factory)
    assert z["loss"][0] == z["loss"][1], "the same forward call: the same value"
    y64, y32 = _yard(c, K, dict(weights=z["weights"]), o, d, jit, target, "ce")
    bound = ml64.bounds(y32, y64)
    names = [k[4:] for k in z if k.startswith("ref:")]
    assert sum(k.startswith("mask:") for k in names) == 10 and len(names) >= 29
    for k in names:
        e = ml64.rel_err(z["got:" + k], z["ref:" + k])
        same = np.array_equal(z["got:" + k], z["ref:" + k])
        print(f"[maskloss] fused against autograd: {k}: error {e:.2e}{', bit-identical' if same else ''}")
        if k.startswith("mask:"):
            assert e <= bound[3], (k, e, bound[3])
        else:
            assert same, (k, e)
    # the shape of the fused call's result, in this process
    rgb_t = _cu(np.random.default_rng(3).random((R, 3)))
    tg = _cu(target, np.int32)
    res = _fused(c, K, o, d, jit, rgb_t, loss_scale=0.25, target_mask=tg, mask_weight=0.5)
    assert len(res) == 3 and res[2].dim() == 0 and float(res[2]) == float(z["loss"][0])
    assert len(_fused(c, K, o, d, jit, rgb_t)) == 2
    res4 = _fused(c, K, o, d, jit, rgb_t, distortion_weight=0.1, target_mask=tg)
    assert len(res4) == 4 and torch.equal(res4[3], res[2])
    c["f"].mask_field = c["mfs"][K]
    try:
        with pytest.raises(NotImplementedError):
            c["f"].render_mse_backward_(T, _cu(o), _cu(d), rgb_t, jitter=_cu(jit))       # the refusal without target_mask stays
    finally:
        c["f"].mask_field = None
    c["model"].zero_grad(set_to_none=True)
    c["mfs"][K].zero_grad(set_to_none=True)
