"""Characteristic loss on the device (csrc/charloss.hip: nvfi_char_loss) against the float64 yardstick tests/char64.py, on the golden fields
A and B of tests/golden/charloss.npz (the velocity net's last layer scaled as the golden script scaled it) and the SH field D of r2.npz.

Bound of every comparison: 4 x the reference's own fp32 error of that quantity against the yardstick, stored per field and quantity in
charloss.npz (`<kind>:ref32_err:<quantity>`: the largest the reference shows over the field's golden cases - the sizes and times below are
not all golden cases).  The factor covers another summation order of the N-term means and of the atomics, nothing more.  The yardstick is
evaluated at the points0 the call returned, so the warp's own error is not part of the comparison; the warp is pinned bit for bit to
field.integrate_pos instead.  Each comparison prints its error / ref32_err ratio (DESIGN 4.15 is where the worst ones are recorded)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import char64 as c64
from conftest import GOLD
from helpers import sh_model          # (the point tests import it from here)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 65, 1000)
ESCAPE_CASE = {"A": "kmax", "B": "out"}
QUANT = list(c64.TERMS) + ["grad:" + n for n in c64.NAMES]


def times_of(K, tmax):
    ts = tmax / (K - 1)
    return [("k1", ts), ("kmax", tmax), ("up", 1.6 * ts), ("zero", 0.0), ("neg", -1.0), ("snap0", 0.3 * ts)]


class Ctx:
    pass


_CTX = {}


def ctx_of(kind):
    """model, yardstick parameters, bounds and the escape-case point set of a field: built once, shared, left unchanged"""
    if kind in _CTX:
        return _CTX[kind]
    from helpers import field_state, make_model
    from nvfi_amd.models.velocity_field import VelBasis
    gc = np.load(os.path.join(GOLD, "charloss.npz"))
    c = Ctx()
    if kind == "D":
        c.model = sh_model()
        src = "A"       # D is field A's geometry with SH shading (make_golden_r2.py): A's reference errors bound it
    else:
        c.model, _ = make_model(kind)
        last = VelBasis.linears(c.model.nvfi.vel_net.weight_net)[-1]
        with torch.no_grad():
            s = float(gc[f"{kind}:vel_scale"])
            last.weight.mul_(s)
            last.bias.mul_(s)
        c.model.nvfi.invalidate_frags()
        src = kind
    c.field = c.model.nvfi
    c.params = c64.params_from_sd(field_state(c.model)[0])
    c.K, c.tmax = int(c.field.num_keyframes), float(c.field.tmax)
    c.tol = {q: 4 * float(gc[f"{src}:ref32_err:{q}"]) for q in QUANT}
    c.points = torch.from_numpy(gc[f"{src}:{ESCAPE_CASE[src]}:points"]).cuda()
    c.ratios = {}
    _CTX[kind] = c
    return c


def grads_of(model):
    from helpers import named_grads
    g = named_grads(model)
    return {n: g[n] for n in c64.NAMES}


def compare(c, label, got_terms, got_grads, y, scale=1.0):
    """both terms and the 13 gradients against the yardstick result y (gradients x scale); prints error / bound per quantity"""
    bad = []
    for i, q in enumerate(c64.TERMS):
        e = c64.rel_err(float(got_terms[i]), y[q])
        r = e / c.tol[q] * 4 if c.tol[q] > 0 else (0.0 if e == 0 else float("inf"))
        c.ratios[q] = max(c.ratios.get(q, 0.0), r)
        print(f"[charloss] {label} {q}: rel err {e:.2e} = {r:.2f} x ref32_err")
        if not e <= c.tol[q]:
            bad.append((q, e, c.tol[q]))
    if got_grads is not None:
        for n in c64.NAMES:
            q = "grad:" + n
            g = got_grads[n]
            g = np.zeros_like(y["grads"][n]) if g is None else g
            e = c64.rel_err(g, scale * y["grads"][n])
            r = e / c.tol[q] * 4 if c.tol[q] > 0 else (0.0 if e == 0 else float("inf"))
            c.ratios[q] = max(c.ratios.get(q, 0.0), r)
            print(f"[charloss] {label} {q}: rel err {e:.2e} = {r:.2f} x ref32_err")
            if not e <= c.tol[q]:
                bad.append((q, e, c.tol[q]))
    assert not bad, (label, bad)


def yardstick(c, pts, points0, t):
    t_k, row = c64.snap_time(c.K, c.tmax, t)
    return c64.char64(c.params, c.K, pts.cpu().numpy(), points0.cpu().numpy(), row), t_k, row


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_yardstick_agreement_and_warp_equality(kind, N):
    c = ctx_of(kind)
    f, pts = c.field, c.points[:N].contiguous()
    for name, t in times_of(c.K, c.tmax):
        c.model.zero_grad(set_to_none=True)
        loss, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
        terms = f.last_char_terms.cpu().numpy()
        assert loss.dim() == 0 and loss.requires_grad
        loss.backward()
        y, t_k, row = yardstick(c, pts, points0, t)
        assert f.characteristic_time(t) == t_k
        # the warp is the stand-alone call's launch path: the same bits
        ref0 = f.integrate_pos(pts, torch.full((N,), t_k, device="cuda"), torch.zeros(N, device="cuda"))
        assert torch.equal(points0, ref0), (kind, N, name)
        np.testing.assert_allclose(float(loss), float(terms[0]) + float(terms[1]), rtol=1e-6)
        if row == 0:
            assert terms[0] == 0.0 and terms[1] == 0.0 and torch.equal(points0, pts)
            assert all(g is None or not g.any() for g in grads_of(c.model).values())
            continue
        compare(c, f"{kind} N={N} {name}", terms, grads_of(c.model), y)
        for k, p in c.model.named_parameters():
            if "vel" in k:
                assert p.grad is None, k
    print(f"[charloss] worst ratios so far ({kind}): " + " ".join(f"{q}={r:.2f}" for q, r in c.ratios.items()))


def call_abi(f, pts, t, weight, grads, want_points0=True):
    """nvfi_char_loss through ctypes: grads = list of 13 tensors / None, or None (value only)"""
    from nvfi_amd import _lib
    L = _lib.lib()
    N = pts.shape[0]
    desc = f._desc()
    nb = C.c_int64(0)
    _lib.check(L.nvfi_char_workspace_bytes(C.byref(desc), C.c_int64(N), C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    terms = torch.full((2,), -7.0, device="cuda")
    p0 = torch.full_like(pts, -7.0) if want_points0 else None
    G = None if grads is None else C.byref(f._grads_struct(list(grads)))
    _lib.check(L.nvfi_char_loss(C.byref(desc), C.c_int64(N), _lib.ptr(pts), C.c_float(t), C.c_float(weight), _lib.ptr(terms), _lib.ptr(p0), G,
                                _lib.ptr(ws), C.c_int64(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return terms.cpu().numpy(), p0


@pytest.mark.parametrize("kind", ["A", "B"])
def test_ctypes_accumulate_skip_and_snap_to_zero(kind):
    c = ctx_of(kind)
    f, pts = c.field, c.points[:65].contiguous()
    ts = c.tmax / (c.K - 1)
    ps = f._render_params()[:13]
    skip = (1, 12)                                  # density_plane_space.1 and basis_mat get a NULL pointer
    bufs = [torch.zeros_like(p) for p in ps]
    sent = [torch.randn_like(p) for p in ps]        # what a skipped tensor's buffer holds, beside the call
    terms, p0 = call_abi(f, pts, ts, 1.0, [None if i in skip else b for i, b in enumerate(bufs)])
    y, _, _ = yardstick(c, pts, p0, ts)
    got = {n: b.detach().cpu().contiguous().numpy() for n, b in zip(c64.NAMES, bufs)}
    for i in skip:
        assert not bufs[i].any()
        got[c64.NAMES[i]] = y["grads"][c64.NAMES[i]]      # (not written: nothing to compare)
    compare(c, f"{kind} abi", terms, got, y)
    # a second call into the same buffers: twice one call
    call_abi(f, pts, ts, 1.0, [None if i in skip else b for i, b in enumerate(bufs)])
    got2 = {n: (b.detach().cpu().contiguous().numpy() if i not in skip else 2 * y["grads"][n]) for i, (n, b) in enumerate(zip(c64.NAMES, bufs))}
    compare(c, f"{kind} abi x2", terms, got2, y, scale=2.0)
    # value only: the same terms, no points0
    terms_v, _ = call_abi(f, pts, ts, 1.0, None, want_points0=False)
    compare(c, f"{kind} abi value-only", terms_v, None, y)
    # a time that snaps to keyframe 0: exact zeros, points0 = points, no buffer changes
    keep = [s.clone() for s in sent]
    terms0, p00 = call_abi(f, pts, 0.3 * ts, 1.0, sent)
    assert terms0[0] == 0.0 and terms0[1] == 0.0 and torch.equal(p00, pts)
    assert all(torch.equal(a, b) for a, b in zip(sent, keep))


@pytest.mark.parametrize("kind", ["A", "B"])
def test_fused_form_weight_and_frozen_tensor(kind):
    c = ctx_of(kind)
    f, pts = c.field, c.points[:63].contiguous()
    t = c.tmax
    frozen = f.app_plane_space[1]
    fname = "app_plane_space.1"
    try:
        # unit-weight autograd call, then (0.3 * loss).backward()
        c.model.zero_grad(set_to_none=True)
        loss, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
        y, _, _ = yardstick(c, pts, points0, t)
        (0.3 * loss).backward()
        compare(c, f"{kind} 0.3 x loss", f.last_char_terms.cpu().numpy(), grads_of(c.model), y, scale=0.3)
        # the fused form with weight 0.3, twice into the same .grad, one tensor frozen with a sentinel .grad
        c.model.zero_grad(set_to_none=True)
        frozen.requires_grad_(False)
        frozen.grad = torch.full_like(frozen, 5.0)
        v = f.characteristic_loss_backward_(pts, t, weight=0.3)
        assert not v.requires_grad and v.dim() == 0
        g1 = grads_of(c.model)
        assert torch.equal(frozen.grad, torch.full_like(frozen, 5.0))
        g1[fname] = 0.3 * y["grads"][fname]
        compare(c, f"{kind} fused w=0.3", f.last_char_terms.cpu().numpy(), g1, y, scale=0.3)
        f.characteristic_loss_backward_(pts, t, weight=0.3)
        g2 = grads_of(c.model)
        assert torch.equal(frozen.grad, torch.full_like(frozen, 5.0))
        g2[fname] = 0.6 * y["grads"][fname]
        compare(c, f"{kind} fused w=0.3 x2", f.last_char_terms.cpu().numpy(), g2, y, scale=0.6)
        # autograd with the frozen tensor: no gradient for it
        c.model.zero_grad(set_to_none=True)
        f.characteristic_loss_at(pts, t).backward()
        assert frozen.grad is None
        g3 = grads_of(c.model)
        g3[fname] = y["grads"][fname]
        compare(c, f"{kind} autograd, one tensor frozen", f.last_char_terms.cpu().numpy(), g3, y)
    finally:
        frozen.requires_grad_(True)
        c.model.zero_grad(set_to_none=True)


def test_arena_mode_scales_into_the_arena_and_accumulates():
    """accumulate_grads_inplace = "arena": with all 13 tensors trainable the backward adds g x (unit-weight gradients) to the head of the
    field's flat gradient buffer in one launch and hands autograd nothing; a second backward accumulates; with one tensor frozen the node
    scales and returns its own gradients instead, and the frozen tensor keeps .grad = None"""
    from nvfi_amd.models.tensorf_keyframe import _rt
    c = ctx_of("A")
    f, pts = c.field, c.points[:63].contiguous()
    t = c.tmax
    frozen = f.app_plane_space[1]
    fname = "app_plane_space.1"
    mode = f.accumulate_grads_inplace
    try:
        f.accumulate_grads_inplace = "arena"
        c.model.zero_grad(set_to_none=True)
        for k in (1, 2):
            loss, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
            y, _, _ = yardstick(c, pts, points0, t)
            (0.3 * loss).backward()
            views = _rt(f)["_arena"]["views"]
            assert all(p.grad is views[id(p)] for p in f._render_params()[:13]), "the gradients are not the arena's views"
            compare(c, f"A arena, backward {k}", f.last_char_terms.cpu().numpy(), grads_of(c.model), y, scale=0.3 * k)
        c.model.zero_grad(set_to_none=True)
        frozen.requires_grad_(False)
        loss, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
        y, _, _ = yardstick(c, pts, points0, t)
        (0.3 * loss).backward()
        assert frozen.grad is None
        g3 = grads_of(c.model)
        g3[fname] = 0.3 * y["grads"][fname]
        compare(c, "A arena, one tensor frozen", f.last_char_terms.cpu().numpy(), g3, y, scale=0.3)
    finally:
        f.accumulate_grads_inplace = mode
        frozen.requires_grad_(True)
        c.model.zero_grad(set_to_none=True)


def untouched_clamp_texels(c, points0, y):
    """per plane parameter name: bool (H, W) - texels a border-clamping rule would touch for out-of-plane taps of the 0 side and that the
    loss, under zero padding, does not depend on (yardstick gradient exactly zero in every channel)"""
    masks = c64.clamped_texels(points0, [int(g) for g in c.field.gridSize.tolist()], c.K)
    out = {}
    for fam in ("density", "app"):
        for key, m in masks.items():
            st, i = key.split(".")
            name = f"{fam}_plane_{st}.{i}"
            sel = m & ~(y["grads"][name][0] != 0).any(0)
            if sel.any():
                out[name] = sel
    return out


@pytest.mark.parametrize("kind", ["A", "B"])
def test_zero_padding_leaves_outside_taps_alone(kind):
    c = ctx_of(kind)
    f, pts = c.field, c.points[:63].contiguous()
    t = c.tmax if kind == "A" else c.tmax / (c.K - 1)
    with torch.no_grad():
        _, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
        before = f.last_char_terms.cpu().numpy()
    assert c64.outside_fraction(points0.cpu().numpy()) > 0
    y, _, _ = yardstick(c, pts, points0, t)
    sel = untouched_clamp_texels(c, points0.cpu().numpy(), y)
    assert sel, "the case has no texel that only a clamped outside tap would touch"
    named = dict(c.model.named_parameters())
    saved = {n: named["nvfi." + n].detach().clone() for n in sel}
    try:
        with torch.no_grad():
            for n, m in sel.items():
                named["nvfi." + n][0][:, torch.from_numpy(m).cuda()] += 1.0
            f.characteristic_loss_at(pts, t)
            after = f.last_char_terms.cpu().numpy()
        print(f"[charloss] {kind} zero padding: {sum(int(m.sum()) for m in sel.values())} texels perturbed, terms {before} -> {after}")
        assert np.array_equal(before, after)
    finally:
        with torch.no_grad():
            for n, v in saved.items():
                named["nvfi." + n].copy_(v)


def test_sh_field():
    c = ctx_of("D")
    f = c.field
    assert f.app_dim == 27
    pts = c.points
    t = c.tmax / (c.K - 1)
    c.model.zero_grad(set_to_none=True)
    loss, points0 = f.characteristic_loss_at(pts, t, return_points0=True)
    loss.backward()
    y, _, _ = yardstick(c, pts, points0, t)
    compare(c, "D (SH) N=1000 k1", f.last_char_terms.cpu().numpy(), grads_of(c.model), y)


def test_use_vel_false_is_refused():
    from helpers import make_model
    from nvfi_amd import _lib
    m, _ = make_model("A", use_vel=False)
    with pytest.raises(_lib.NvfiError, match="use_vel"):
        m.nvfi.characteristic_loss(16, 0.25)
