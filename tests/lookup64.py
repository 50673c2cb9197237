"""Float64 restatement, with autograd, of the differentiable field lookups (include/nvfi_hip.h: nvfi_density_grad, nvfi_appfeat_at,
nvfi_appfeat_grad; TensorVMKeyframeTimeKplane.lookup_density / lookup_appfeature; reference compute_densityfeature / compute_appfeature,
models/tensorf_keyframe.py:233-310, under autograd): the yardstick of tests/test_lookup_golden.py (against the reference's goldens) and of
tests/test_gpu_lookup.py (against the device).

  density     feat = sum_c prod_i space_i(x_a, x_b)[c] time_i(x_c, t')[c]
  appearance  feat = basis_mat (prod_i space_i time_i)
  every plane lookup is bilinear F.grid_sample(align_corners=True, padding_mode="zeros"), the time planes included: t' is
  per point, may be fractional and may lie outside [-1, 1].  The gradients are those of sum(feat * g): to the twelve planes, to basis_mat.weight
  and to the four columns of xyzt (ATen's grid_sampler_2d_backward: the difference of the in-range taps times (W - 1) / 2, (H - 1) / 2, and
  (K - 1) / 2 for t').

The product over the planes is render64._planes' (same plane pairs, same order; `planes` below is that function with the lookup restated, and
tests/test_lookup_golden.py holds the two against each other), the parameters are a render64.Field's.  Like the other yardsticks, what is fixed
before the planes are touched - the points - stays fp32-rounded and is then promoted, and the discrete decisions are taken on fp32 values: the CELL
of a lookup (the floor of the texel coordinate and the in-range mask of each tap) is common.h's bl_setup_xy expression on the fp32 coordinate,
(g + 1) * ((W - 1) / 2) in float32, floor, clamp to [-4, W + 2], NaN -> -4; the weights are the `dtype` texel coordinate minus that floor.  Where the
fp32 coordinate rounds onto a texel node that the exact one misses by 1e-7, the weight leaves [0, 1) by as much: the value is continuous there, and
the gradient is the one of the cell the device reads.  A lookup none of whose taps is in range (far or non-finite coordinates) is exactly zero with
zero gradients.  dtype=float32 is a plain fp32 implementation of the same statement: the floor the bounds are derived from.

One deliberately wrong variant each (`wrong=True`), values untouched: density - the t' gradient scaled by K / 2 instead of (K - 1) / 2;
appearance - the share of a space plane (and of the coordinates through it) leaves the time plane of the same index out of its other-five product."""
import numpy as np
import torch

import render64 as r64

D_NAMES = r64.PLANE_NAMES[:6]
A_NAMES = r64.PLANE_NAMES[6:] + ["basis_mat.weight"]


def _cell(g32, W):
    """bl_setup_xy on one axis in float32: (floor of the texel coordinate (float32, unclamped), cell index, tap 0 in range, tap 1 in range)"""
    x = (g32 + 1.0) * np.float32((W - 1) / 2.0)
    xf = torch.floor(x)
    c = torch.clamp(xf, -4.0, float(W + 2))
    c = torch.where(c == c, c, torch.full_like(c, -4.0))
    x0 = c.to(torch.int64)
    return xf, x0, (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)


def bilinear(P, g):
    """(C, n): the plane P (1, C, H, W) in `dtype` at the grid coordinates g (n, 2) = (x, y) in `dtype`, cell taken in float32"""
    C, H, W = P.shape[1:]
    dtype = P.dtype
    g32 = g.detach().to(torch.float32)
    xf, x0, xi0, xi1 = _cell(g32[:, 0], W)
    yf, y0, yi0, yi1 = _cell(g32[:, 1], H)
    m = [xi0 & yi0, xi1 & yi0, xi0 & yi1, xi1 & yi1]
    live = m[0] | m[1] | m[2] | m[3]
    zero = torch.zeros_like(g[:, 0])
    gx, gy = torch.where(live, g[:, 0], zero), torch.where(live, g[:, 1], zero)          # (a dead lookup may hold NaN: kept out of the graph)
    w = (gx + 1.0) * ((W - 1) / 2.0) - torch.where(live, xf, torch.zeros_like(xf)).to(dtype)
    n = (gy + 1.0) * ((H - 1) / 2.0) - torch.where(live, yf, torch.zeros_like(yf)).to(dtype)
    e, s = 1.0 - w, 1.0 - n
    flat = P.reshape(C, H * W)
    out = None
    for k, (dx, dy, wt) in enumerate(((0, 0, e * s), (1, 0, w * s), (0, 1, e * n), (1, 1, w * n))):
        idx = (y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)
        term = flat[:, idx] * (wt * m[k].to(dtype))
        out = term if out is None else out + term
    return out


def planes(P, which, x4, wrong=False):
    """render64._planes with the lookup restated (`bilinear`): (C, n) prod_i space_i * time_i"""
    out = None
    for i in range(3):
        a = bilinear(P[f"{which}_plane_space.{i}"], x4[:, list(r64.MAT_SPACE[i])])
        b = bilinear(P[f"{which}_plane_time.{i}"], x4[:, list(r64.MAT_TIME[i])])
        ab = a * b
        if wrong:                                   # same value; d / d a = 1 instead of b
            ab = a.detach() * b + (a - a.detach())
        out = ab if out is None else out * ab
    return out


def _run(field, names, xyzt, g, dtype, device, feat_of):
    P = {k: field.p32[k].to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    q = torch.as_tensor(np.array(np.asarray(xyzt, np.float32), copy=True)).reshape(-1, 4).to(device=device, dtype=dtype).requires_grad_(True)
    feat = feat_of(P, q)
    out = dict(value=feat.detach().cpu().numpy())
    if g is not None:
        gt = torch.as_tensor(np.asarray(g, np.float32)).reshape(feat.shape).to(device=device, dtype=dtype)
        grads = torch.autograd.grad((feat * gt).sum(), [q] + [P[k] for k in names], allow_unused=True)
        out["g_xyzt"] = (torch.zeros_like(q) if grads[0] is None else grads[0]).cpu().numpy()
        out["grads"] = {k: (torch.zeros_like(P[k]) if gr is None else gr).cpu().numpy() for k, gr in zip(names, grads[1:])}
    return out


def density_lookup64(field, xyzt, g=None, dtype=torch.float64, device="cpu", wrong=False):
    """dict: value (n,), and with g (n,) = d loss / d feat: g_xyzt (n, 4), grads {name: (1, 24, H, W)} of the six density planes"""
    out = _run(field, D_NAMES, xyzt, g, dtype, device, lambda P, q: planes(P, "density", q).sum(0))
    if wrong and g is not None and field.K > 1:
        out["g_xyzt"][:, 3] *= field.K / (field.K - 1.0)
    return out


def app_lookup64(field, xyzt, g=None, dtype=torch.float64, device="cpu", wrong=False):
    """dict: value (n, app_dim), and with g (n, app_dim): g_xyzt (n, 4), grads of the six appearance planes and basis_mat.weight"""
    return _run(field, A_NAMES, xyzt, g, dtype, device,
                lambda P, q: torch.nn.functional.linear(planes(P, "app", q, wrong=wrong).T, P["basis_mat.weight"]))


def tensors(y):
    """{label: array} of a result: value, g_xyzt and every parameter gradient"""
    out = {"value": y["value"]}
    if "g_xyzt" in y:
        out["g_xyzt"] = y["g_xyzt"]
        out.update({"grad:" + k: v for k, v in y["grads"].items()})
    return out


def bound(ref64, ref32):
    """the rule of every comparison: max(3 x the float32 floor of the case, 1e-5 x max |ref64|), absolute, per tensor"""
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    if not ref64.size:
        return 0.0
    return max(3.0 * float(np.abs(ref32 - ref64).max()), 1e-5 * float(np.abs(ref64).max()))


def max_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) if ref.size else 0.0


def texel_distance(xyzt, grid, K):
    """(n, 4): per coordinate, the distance of its fp32 texel coordinate from the nearest integer (the fp32 expression of the device)"""
    q = np.asarray(xyzt, np.float32).reshape(-1, 4)
    out = np.empty(q.shape, np.float64)
    for c, W in enumerate(list(grid) + [K]):
        x = (q[:, c] + np.float32(1)) * np.float32((W - 1) / 2.0)
        out[:, c] = np.abs(x.astype(np.float64) - np.rint(x.astype(np.float64)))
    return out


def point_mix(rng, n, grid, K, extent=1.15, n_nodes=None):
    """the golden-style mix of n points (n, 4) float32: interior points, exact texel nodes (-1, +1, 0 where G is odd), box faces, points out to
    `extent` x the box, integer and fractional time rows, t' below -1 and above +1.  The special points come first, so that a short prefix holds
    them; every OTHER coordinate keeps its fp32 texel coordinate at least 1e-3 from an integer (redrawn until it does)."""
    special = []
    for c in range(3):
        for v in (-1.0, 1.0) + ((0.0,) if grid[c] % 2 else ()):
            special.append((c, v))
    special += [(3, -1.0), (3, 1.0), (3, -1.2), (3, 1.25)]
    special = special[:min(len(special) if n_nodes is None else n_nodes, n)]
    scale = np.tile(np.array([extent, extent, extent, 1.3], np.float32), (n, 1))
    scale[:len(special), :3] = 0.9                          # the other coordinates of a special point stay inside the box
    q = (rng.random((n, 4)) * 2 - 1).astype(np.float32) * scale
    rows = (2.0 * rng.integers(0, K, n) / max(K - 1, 1) - 1.0).astype(np.float32)
    on_row = rng.random(n) < 0.3
    q[on_row, 3] = rows[on_row]
    for _ in range(64):
        bad = texel_distance(q, grid, K) < 1e-3
        bad[on_row, 3] = False
        if not bad.any():
            break
        fresh = (rng.random(q.shape) * 2 - 1).astype(np.float32) * scale
        q[bad] = fresh[bad]
    assert not bad.any()
    for i, (c, v) in enumerate(special):
        q[i, c] = np.float32(v)
    return q
