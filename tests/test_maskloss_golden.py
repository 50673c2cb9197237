"""tests/maskloss64.py (the float64 yardstick of the mask loss, nvfi_mask_loss_fwd / nvfi_mask_loss_bwd) on the CPU, fields A and B, on the rays,
jitter and weight map of tests/golden/flowloss.npz - the REFERENCE's own train-mode render (tests/golden/make_golden_flowloss.py) - with the
MaskFields of maskfield64.params_for.

What is checked here:
  - an independent statement: the value and the ten gradients of the yardstick against MaskField's own yardstick (maskfield64.mask64) fed the
    entries' g_mask = w_j g_q[ray(j)] formed in numpy from the yardstick's mask map, and g_weights against sum_k g_q m in numpy;
  - the plain-fp32 floors: maskloss64(float32) against maskloss64(float64), under maskloss64.CPU_D32_MAX;
  - the ReLU-kink share of the rays tests/test_gpu_maskloss.py renders (maskloss64.gpu_rays, the same rays and jitter seeds) stays under
    maskfield64.KINK_CAP on the CPU float32 run of the yardstick alone (render64's fp32 weights standing in for the device's);
  - the yardstick moves when it should: one list entry dropped, two labels swapped, a background ray, ignored rays, every ray ignored.
  - the reference: tests/golden/maskloss.npz + maskloss_grads_*.npz, the REFERENCE's own train-mode render_pts with its MaskField attached, the
    contract's loss on its mask_map in torch fp32 and autograd.grad (tests/golden/make_golden_maskloss.py), cases c0 .. c5.  The golden tensors
    are fp32, one plain-fp32 evaluation away from the float64 yardstick: they may differ from it by maskloss64.bounds, max(3 x the float32
    distance measured here, the floor).  Rays with a masked sample near a MaskField kink or the weight threshold are ignored in every case."""
import os

import numpy as np
import pytest
import torch

import maskfield64 as m64
import maskloss64 as ml64
import render64 as r64
from conftest import GOLD
from helpers import load_meta

T = 19.0 / 60.0
EPS = 1e-5
CASES = [(kind, K, lk, soft) for kind in "AB" for K in (2, 8, 17, 32) for lk in ("ce", "l2") for soft in (False, True)]


@pytest.fixture(autouse=True)
def four_threads():
    """the order of torch's fp32 matrix sums, and with it the measured floor, follows the thread count"""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def data():
    z = np.load(os.path.join(GOLD, "flowloss.npz"))
    out = {}
    for kind in "AB":
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        p = kind + ":"
        n = 48                              # the first rays of the fixture: a few hundred entries
        out[kind] = dict(field=r64.Field(sd, meta), o=z[p + "rays_o"][:n], d=z[p + "rays_d"][:n], u=z[p + "u"].reshape(-1)[:n], w=z[p + "weight"][:n])
    return out


def _target(R, K, soft):
    rng = np.random.default_rng(5 + R + 100 * K)
    if not soft:
        lab = rng.integers(0, K, R).astype(np.int32)
        lab[1], lab[2] = K, -1
        return lab
    y = rng.random((R, K)).astype(np.float32)
    y = y / y.sum(1, keepdims=True) * rng.random((R, 1)).astype(np.float32)
    y[1] = 0.0
    y[2, K - 1] = np.nan
    return y.astype(np.float32)


def _run(c, K, lk, target, **kw):
    return ml64.maskloss64(c["field"], m64.params_for(K), c["o"], c["d"], T, c["w"], c["u"], target, kind=lk, eps=EPS, **kw)


_worst = [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("kind,K,lk,soft", CASES)
def test_yardstick_against_its_parts_and_the_fp32_floor(data, kind, K, lk, soft):
    c = data[kind]
    R = len(c["o"])
    target = _target(R, K, soft)
    y64 = _run(c, K, lk, target)
    y32 = _run(c, K, lk, target, dtype=torch.float32, want_margin=False)
    assert y64["M"] > 128 and y64["n"] == R - 1 and y32["n"] == y64["n"] and y64["loss"] > 0
    # the same statement from its parts, in numpy float64
    y, ok = ml64.targets(target, R, K)
    q = y64["mask_map"]
    ray, smp = y64["idx"][:, 0], y64["idx"][:, 1]
    n = y64["n"]
    e32 = float(np.float32(EPS))
    if lk == "l2":
        loss = (((q - y) ** 2) * ok[:, None]).sum() / (2 * n * K)
        gq = (q - y) / (n * K) * ok[:, None]
    else:
        loss = (np.where(y != 0, -y * np.log(q + e32), 0.0) * ok[:, None]).sum() / n
        gq = np.where(y != 0, -y / (q + e32), 0.0) / n * ok[:, None]
    assert abs(loss - y64["loss"]) <= 1e-12 * abs(loss)
    own = ml64.d32(y32, y64)
    for i in range(4):
        _worst[i] = max(_worst[i], own[i])
    print(f"[maskloss cpu] {kind}:K={K}:{lk}:{'soft' if soft else 'labels'}: M={y64['M']} loss {y64['loss']:.6g}; fp32 distance: mask_map {own[0]:.2e}, "
          f"loss {own[1]:.2e}, g_weights {own[2]:.2e}, worst gradient {own[3]:.2e}; worst so far {_worst}")
    for i, what in enumerate(("mask_map", "loss", "g_weights", "worst gradient")):
        assert own[i] <= ml64.CPU_D32_MAX[i], (what, own[i], ml64.CPU_D32_MAX[i])
    assert not y64["g_weights"][~y64["mask"]].any() and not y64["g_weights"][~ok].any()
    if not soft:
        assert not y64["g_weights"][1].any() or lk == "l2"          # a background ray: no ce gradient; l2 pulls its q to zero


@pytest.mark.parametrize("kind", "AB")
def test_gradients_are_maskfields_own(data, kind):
    """the ten gradients are MaskField's (maskfield64.mask64, pinned to the reference by tests/test_maskfield64_golden.py) at the yardstick's
    positions under g_mask = w_j g_q[ray(j)]; g_weights = sum_k g_q m"""
    c = data[kind]
    K, R = 8, len(c["o"])
    target = _target(R, K, False)
    y64 = _run(c, K, "ce", target)
    y, ok = ml64.targets(target, R, K)
    ray, smp = y64["idx"][:, 0], y64["idx"][:, 1]
    w = c["w"].astype(np.float64)[ray, smp]
    x32 = y64["x"].astype(np.float32)
    # (mask64 takes fp32 points: evaluate the yardstick on the same rounded points)
    y64p = _run(c, K, "ce", target, points=x32)
    gq = np.where(y != 0, -y / (y64p["mask_map"] + float(np.float32(EPS))), 0.0) / y64p["n"] * ok[:, None]
    g = w[:, None] * gq[ray]
    part = m64.mask64(m64.params_for(K), x32, g)
    # mask64 rounds g to fp32: the comparison carries that rounding
    for k in ml64.GRAD_KEYS:
        assert ml64.rel_err(y64p[k], part[k]) < 5e-7, k
    gw = (gq[ray] * part["mask"]).sum(1)
    assert np.abs(y64p["g_weights"][ray, smp] - gw).max() <= 1e-12 * np.abs(gw).max()


@pytest.mark.parametrize("kind", "AB")
def test_yardstick_moves(data, kind):
    c = data[kind]
    K, R = 8, len(c["o"])
    target = _target(R, K, False)
    y64 = _run(c, K, "ce", target, want_margin=False)
    b = ml64.bounds(_run(c, K, "ce", target, dtype=torch.float32, want_margin=False), y64)
    cut = y64["mask"].copy()
    r, s = y64["idx"][-1]
    cut[r, s] = False
    ycut = _run(c, K, "ce", target, mask=cut, want_margin=False)
    assert ycut["M"] == y64["M"] - 1 and max(ml64.rel_err(ycut[k], y64[k]) for k in ml64.GRAD_KEYS) > b[3]
    sw = target.copy()
    i, j = [r for r in range(R) if 0 <= target[r] < K and y64["mask"][r].any()][:2]
    if sw[i] == sw[j]:
        sw[j] = (sw[j] + 1) % K
    sw[i], sw[j] = sw[j], sw[i]
    ysw = _run(c, K, "ce", sw, want_margin=False)
    assert abs(ysw["loss"] - y64["loss"]) > b[1] * abs(y64["loss"]) and ml64.rel_err(ysw["g_weights"], y64["g_weights"]) > b[2]
    none = _run(c, K, "ce", np.full(R, -1, np.int32), want_margin=False)
    assert none["n"] == 0 and none["loss"] == 0.0 and not none["g_weights"].any() and not any(none[k].any() for k in ml64.GRAD_KEYS)
    above = target.copy()
    above[0] = K + 1                                                   # a label above K: ignored, as the device treats it
    assert _run(c, K, "ce", above, want_margin=False)["n"] == y64["n"] - 1


@pytest.mark.parametrize("R", ml64.GPU_SHAPES)
@pytest.mark.parametrize("kind", "AB")
def test_kink_share_of_the_gpu_tests_rays(gold, data, kind, R):
    """the rays and the jitter of tests/test_gpu_maskloss.py (maskloss64.gpu_rays) through the float32 run of the yardstick alone, on render64's own
    fp32 training weights: the share of masked entries within one rounding bound of a MaskField ReLU kink meets the cap"""
    o, d, jit = ml64.gpu_rays(gold, kind, R)
    share, low, M = ml64.kink_share(data[kind]["field"], o, d, jit, T)
    print(f"[maskloss cpu] {kind}:R={R}: M={M}, entries with margin < 1: {low} ({share:.4f}), cap {m64.KINK_CAP}")
    assert M > 0 and share <= m64.KINK_CAP
    if R <= 2:
        assert low == 0


GOLD_CASES = [f"{kind}:c{i}" for kind in "AB" for i in range(6)]


@pytest.fixture(scope="module")
def ml_gold():
    z = dict(np.load(os.path.join(GOLD, "maskloss.npz")))
    for fn in ("maskloss_grads_A1.npz", "maskloss_grads_A2.npz", "maskloss_grads_B1.npz", "maskloss_grads_B2.npz"):
        assert os.path.getsize(os.path.join(GOLD, fn)) < (1 << 20), fn
        z.update(np.load(os.path.join(GOLD, fn)))
    assert os.path.getsize(os.path.join(GOLD, "maskloss.npz")) < (1 << 20)
    return z


@pytest.mark.parametrize("case", GOLD_CASES)
def test_yardstick_matches_reference(ml_gold, data, case):
    z, kind, name = ml_gold, case[0], case[2:]
    fl = np.load(os.path.join(GOLD, "flowloss.npz"))
    field = data[kind]["field"]
    o, d, u = fl[kind + ":rays_o"], fl[kind + ":rays_d"], z[kind + ":u"]
    R, S = len(o), field.S
    mask = np.unpackbits(z[kind + ":mask"])[:R * S].astype(bool).reshape(R, S)
    w = np.zeros((R, S), np.float32)
    w[mask] = z[kind + ":weight_masked"]
    bad = z[kind + ":ignored"]
    K, lk, target = int(z[case + ":K"]), str(z[case + ":kind"]), z[case + ":target"]
    a = (field, m64.params_for(K), o, d, T, w, u, target)
    y64 = ml64.maskloss64(*a, kind=lk, eps=EPS, mask=mask)
    y32 = ml64.maskloss64(*a, kind=lk, eps=EPS, mask=mask, dtype=torch.float32, want_margin=False)
    assert y64["M"] == int(z[case + ":M"]) and y64["n"] == int(z[case + ":n"])
    counted = ~bad[y64["idx"][:, 0]]
    assert (y64["margin"][counted] >= m64.KINK_MARGIN).all()
    assert not (np.abs(z[kind + ":weight_masked"].astype(np.float64) - field.thres)[counted] <= 4 * float(np.spacing(np.float32(field.thres)))).any()
    own, bound = ml64.d32(y32, y64), ml64.bounds(y32, y64)
    for i, what in enumerate(("mask_map", "loss", "g_weights", "worst gradient")):
        assert own[i] <= max(float(z[case + ":floor"][i]) * 1.02, ml64.CPU_D32_MAX[i]), (case, what, own[i])
    gw = np.zeros((R, S), np.float32)
    gw[mask & ~bad[:, None]] = z[case + ":g_weights"]
    got = dict(mask_map=z[case + ":mask_map"], loss=float(z[case + ":loss"]), g_weights=gw)
    if name == "c4":
        assert y64["n"] == 0 and y64["loss"] == 0.0 and got["loss"] == 0.0 and not gw.any() and not any(y64[k].any() for k in ml64.GRAD_KEYS)
        assert ml64.rel_err(got["mask_map"], y64["mask_map"]) <= bound[0]
        return
    for k in ml64.GRAD_KEYS:
        got[k] = z[f"{case}:{k}"]
    err = ml64.d32(got, y64)
    print(f"[maskloss golden] {case}: {lk} K={K} M={y64['M']} n={y64['n']}: reference against the yardstick {err}, bounds {bound}, fp32 yardstick {own}")
    for i, what in enumerate(("mask_map", "loss", "g_weights", "worst gradient")):
        assert err[i] <= bound[i], (case, what, err[i], bound[i])
    if name == "c3":
        assert y64["n"] == int((~bad).sum()) - 3 and int((target == K).sum()) == 1
