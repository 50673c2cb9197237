"""The float64 yardstick of MaskField (tests/maskfield64.py) on the CPU: pinned to the goldens generated from the reference (tests/golden/maskfield.npz:
K8 with 333 points, K3 with 65), and what the yardstick would see of a kernel that skips work, on the very arrays tests/test_gpu_maskfield64.py uploads.

Pin: the reference IS a plain fp32 evaluation, so the yardstick must agree with it within 3 x the distance of the yardstick's own float32 evaluation
on the same inputs (mask: max abs; gradients: max(maxrel, rel_l2)), computed here and printed.

Blind spots, per cell of maskfield64.MATRIX, as multiples of the cell's own bound (the gradient of (mask * g).sum() is a sum over the points, so
"a kernel that loses points" is the yardstick minus the yardstick of those points alone):
  the last point lost: every gradient tensor moves by > 100 x its bound (N > 1; K > 1: at K = 1 every gradient is exactly zero);
  the last 32-point tile lost (N >= 8193): the same;
  g[:, K-1] read as zero (K > 1): mask_fc.weight moves by > 100 x its bound in every cell of K's own head; under the steep heads, where the
      softmax leaves the last class next to nothing at most points, by 51 x (K = 17) and more, asserted > 10 x;
  head rows j and 16 + j swapped (K > 16, every j with 16 + j < K): the mask moves by > 100 x its bound in every cell of K's own head.  A steep
      head leaves some pairs of classes next to nothing at all 129 points (K = 32: rows 3 / 19 move the mask by 6 x the bound): there only the
      best-seen pair is asserted, the figures are printed, and the steep cells are not what pins the row order.
Gate flips (maskfield64.gate_flips / admit_flips: what the GPU test admits on the large cells) are found where they are and hide no lost point.
The kink cap of maskfield64.points holds for every large case, the small cases hold no point with margin < 4; at K = 1 the yardstick's mask is
exactly 1.0 and every gradient exactly 0; the float32 figures stay under maskfield64.MAX_D32 (FLOOR_G = 3 x that), printed per group."""
import numpy as np
import pytest
import torch

import maskfield64 as m64

CELLS = [pytest.param(K, N, steep, id=f"K{K}-N{N}" + ("-steep" if steep else "")) for K, N, steep in m64.MATRIX]


@pytest.mark.parametrize("tag", ["K8", "K3"])
def test_yardstick_matches_the_reference(tag):
    z = m64._gold()
    p, x, g = m64.gold_params(tag, z), z[f"{tag}:pts"], z[f"{tag}:g"]
    y64, y32 = m64.mask64(p, x, g), m64.mask64(p, x, g, dtype=torch.float32)
    d = m64.d32(y32, y64)
    e = float(np.abs(z[f"{tag}:mask"].astype(np.float64) - y64["mask"]).max())
    print(f"[maskfield64] {tag}: mask reference {e:.2e}, float32 evaluation {d['mask']:.2e}, bound {3 * d['mask']:.2e}")
    assert y64["mask"].shape == z[f"{tag}:mask"].shape and e <= 3 * d["mask"]
    for k in m64.GRAD_KEYS:
        e = m64.err(z[f"{tag}:grad:{k}"], y64[k])
        print(f"[maskfield64] {tag}: {k}: reference {e:.2e}, float32 evaluation {d[k]:.2e}, bound {3 * d[k]:.2e}")
        assert y64[k].shape == z[f"{tag}:grad:{k}"].shape and e <= 3 * d[k], (tag, k, e, d[k])


def test_params_for():
    z = m64._gold()
    for K in (1, 5, 8, 9, 32):
        p = m64.params_for(K)
        assert [a.shape for a in p[:8]] == [(128, 3), (128,)] + [(128, 128), (128,)] * 3 and p[8].shape == (K, 128) and p[9].shape == (K,)
        assert all(a.dtype == np.float32 for a in p)
        for a, b in zip(p[:8], m64.gold_params("K8", z)[:8]):
            assert np.array_equal(a, b)
        assert np.array_equal(p[8][:8], z["K8:sd:mask_fc.weight"][:min(K, 8)]) and np.array_equal(p[9][:8], z["K8:sd:mask_fc.bias"][:min(K, 8)])
    w = np.abs(z["K8:sd:mask_fc.weight"]).max()
    p = m64.params_for(32)
    assert np.abs(p[8][8:]).max() <= w and np.abs(p[8][8:]).max() > 0.9 * w and len(np.unique(p[8][8:])) > 2000
    s = m64.params_for(17, steep=True)
    assert np.array_equal(s[8], m64.params_for(17)[8] * np.float32(32)) and np.array_equal(s[9], m64.params_for(17)[9] * np.float32(32))
    with pytest.raises(ValueError):
        m64.params_for(33)


def test_k1_is_exact():
    y64, y32, _ = m64.yardstick(1, m64.N_SMALL)
    for y in (y64, y32):
        assert (y["mask"] == 1.0).all() and y["mask"].shape == (m64.N_SMALL, 1)
        for k in m64.GRAD_KEYS:
            assert not y[k].any(), k


@pytest.mark.parametrize("N", sorted({N for _, N, _ in m64.MATRIX}))
def test_kinks(N):
    trunk = m64.params_for(1)
    for K in sorted({K for K, n, _ in m64.MATRIX if n == N}):
        mg = m64.margin(trunk, m64.case(K, N)[1])
        if N <= 129:
            assert mg.min() >= m64.KINK_MARGIN, (K, N, mg.min())
        else:
            share = float((mg < 1.0).mean())
            print(f"[maskfield64] K{K} N{N}: {share:.2%} of the points within one rounding bound of a kink (cap {m64.KINK_CAP:.1%})")
            assert share <= m64.KINK_CAP, (K, N, share)


def test_margin_sees_a_kink():
    """a point moved onto the zero of a first-layer unit has margin ~0; scaling the inputs leaves a margin unchanged only in the first layer"""
    p = m64.params_for(1)
    W, b = p[0].astype(np.float64), p[1].astype(np.float64)
    x = np.array([[0.3, -0.2, 0.1]])
    j = 5
    x = x - (W[j] @ x[0] + b[j]) / (W[j] @ W[j]) * W[j]            # onto the plane z_j = 0
    assert m64.margin(p, x.astype(np.float32))[0] < 1.0
    assert m64.margin(p, np.array([[0.9, 0.9, 0.9]], np.float32))[0] > 0


def _moved(full, part, bound):
    """by how many bounds each gradient tensor of the yardstick moves when the contribution `part` is lost"""
    return {k: m64.err(full[k] - part[k], full[k]) / bound[k] for k in m64.GRAD_KEYS}


_group = {}


@pytest.mark.parametrize("K,N,steep", CELLS)
def test_blind_spots(K, N, steep):
    p, x, g = m64.case(K, N, steep)
    y64, y32, bound = m64.yardstick(K, N, steep)
    d = m64.d32(y32, y64)
    dg = max(d[k] for k in m64.GRAD_KEYS)
    w = _group.setdefault(m64.group(K, N, steep), [0.0, 0.0])
    w[0], w[1] = max(w[0], d["mask"]), max(w[1], dg)
    print(f"[maskfield64] K{K} N{N}{' steep' if steep else ''}: float32 evaluation: mask {d['mask']:.2e} abs, gradients {dg:.2e}")
    assert dg <= 1.5 * m64.MAX_D32, ("FLOOR_G is stale: a float32 figure above MAX_D32", K, N, steep, dg)
    assert y64["mask"].shape == (N, K) and abs(y64["mask"].sum(1) - 1.0).max() < 1e-14
    if K == 1:
        return
    if N > 1:
        m = _moved(y64, m64.mask64(p, x[-1:], g[-1:]), bound)
        print(f"  last point lost: {min(m.values()):.0f} .. {max(m.values()):.0f} x the bound")
        assert min(m.values()) > 100.0, ("last point", m)
    if N >= 8193:
        m = _moved(y64, m64.mask64(p, x[-32:], g[-32:]), bound)
        print(f"  last tile lost: {min(m.values()):.0f} .. {max(m.values()):.0f} x the bound")
        assert min(m.values()) > 100.0, ("last tile", m)
    g0 = g.copy()
    g0[:, K - 1] = 0.0
    m = m64.err(m64.mask64(p, x, g0)["mask_fc.weight"], y64["mask_fc.weight"]) / bound["mask_fc.weight"]
    print(f"  g[:, K-1] read as zero: mask_fc.weight moves by {m:.0f} x the bound")
    assert m > (10.0 if steep else 100.0), ("last class of g", m)
    swaps = []
    for j in range(K - 16):
        q = [a.copy() for a in p]
        q[8][[j, 16 + j]], q[9][[j, 16 + j]] = p[8][[16 + j, j]], p[9][[16 + j, j]]
        swaps.append(float(np.abs(m64.mask64(q, x)["mask"] - y64["mask"]).max()) / bound["mask"])
    if swaps:
        print(f"  head rows j / 16 + j swapped, j < {K - 16}: the mask moves by {min(swaps):.0f} .. {max(swaps):.0f} x the bound")
        assert steep or min(swaps) > 100.0, ("head rows swapped", swaps)
        assert max(swaps) > 100.0


def test_gate_flips_are_found_and_hide_nothing():
    """K = 8, N = 8193: the float32 evaluation with two listed gates taken the other way is told apart from the yardstick, admit_flips names exactly
    those two and the rest is back inside the bound; the float32 evaluation itself takes none; a lost last point or tile is explained by no choice
    of gates (still > 100 x the bound after whatever admit_flips takes)"""
    K, N = 8, 8193
    p, x, g = m64.case(K, N)
    y64, y32, bound = m64.yardstick(K, N)
    flips = m64.gate_flips(p, x, g)
    share = len({t[0] for t, _ in flips}) / N
    print(f"[maskfield64] K{K} N{N}: {len(flips)} gates within one rounding bound of their kink, on {share:.2%} of the points")
    assert 0 < share <= m64.KINK_CAP
    assert m64.admit_flips(y32, y64, flips)[1] == []
    big = sorted(range(len(flips)), key=lambda n: -max(np.abs(flips[n][1][k]).max() / np.abs(y64[k]).max() for k in m64.GRAD_KEYS))[:2]
    got = {k: y32[k].astype(np.float64) + flips[big[0]][1][k] + flips[big[1]][1][k] for k in m64.GRAD_KEYS}
    assert max(m64.err(got[k], y64[k]) / bound[k] for k in m64.GRAD_KEYS) > 10.0
    ref, taken = m64.admit_flips(got, y64, flips)
    assert sorted(taken) == sorted(flips[n][0] for n in big), taken
    for k in m64.GRAD_KEYS:
        assert m64.err(got[k], ref[k]) <= bound[k], k
    for cut in (1, 32):
        part = m64.mask64(p, x[-cut:], g[-cut:])
        lost = {k: y64[k] - part[k] for k in m64.GRAD_KEYS}
        ref, taken = m64.admit_flips(lost, y64, flips)
        m = min(m64.err(lost[k], ref[k]) / bound[k] for k in m64.GRAD_KEYS)
        print(f"  last {cut} point(s) lost: {len(taken)} gates taken, still {m:.0f} x the bound")
        assert m > 100.0


def test_float32_figures_per_group():
    """(after the cells: prints the table that the docstring of tests/test_gpu_maskfield64.py and DESIGN carry)"""
    for K, N, steep in m64.MATRIX:
        y64, y32, _ = m64.yardstick(K, N, steep)
        d = m64.d32(y32, y64)
        w = _group.setdefault(m64.group(K, N, steep), [0.0, 0.0])
        w[0], w[1] = max(w[0], d["mask"]), max(w[1], max(d[k] for k in m64.GRAD_KEYS))
    for grp, (a, b) in sorted(_group.items()):
        print(f"[maskfield64] float32 evaluation, {grp[0]:7s} {grp[1]:7s}: mask {a:.2e} abs, gradients {b:.2e}")
    assert max(b for _, b in _group.values()) <= 1.5 * m64.MAX_D32          # (1.5: another CPU's fp32 sums; beyond that FLOOR_G is stale)
    assert max(a for (kg, _), (a, _) in _group.items() if kg != "steep") <= m64.MASK_FLOOR / 3
