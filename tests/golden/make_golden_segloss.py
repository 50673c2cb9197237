#!/usr/bin/env python
"""Golden vectors of the segmentation objective, generated from the REFERENCE implementation (utils/seg_loss.py, PyTorch CPU, fp32):
    python tests/golden/make_golden_segloss.py        (NVFI_REFERENCE: checkout of the reference; default as in make_golden.py)
The reference module imports pytorch3d.ops for its neighbour search.  That package is not needed for anything else, so this script installs a
small shim of its own in sys.modules: brute-force `knn_points` (squared distances, ascending, stable - equal distances keep the lower index
first, the point itself included) and `knn_gather`.  The golden's neighbour tables are therefore the shim's.

Writes tests/golden/segloss.npz.  Per case: inputs (pc, flow, mask), the reference's three losses, R, t, and - per point - pc_transformed,
idx and d loss / d mask of each loss.  To keep the file under 1 MiB the per-point outputs of the two large cases are stored for every
ROW_STRIDE-th point (`<case>:rows`); the idx of case `lattice_k4` is stored in full.  Cases:
  lattice_k4    a jittered 64^3 lattice (tensor-product jitter, as sample_volume_points draws it) cut to a shell, N ~ 9 000, K = 8, softmax masks
                of a random MLP, flow = two rigid motions + noise; smooth_loss(k=4, radius=0.01) as train_segm.py:193 calls it
  lattice_k16   the same cloud, the function defaults k=16, radius=0.1 with loss_norm=2 (shares inputs and the dynamic / entropy outputs)
  small         N = 257, K = 3, a random cloud sparse enough that many slots lie beyond the radius
  zerocol       a mask with one all-zero column: 0 / 0 -> NaN -> the identity branch of fit_motion_svd_batch
It also checks what the tests rely on and prints the figures that tests/test_segloss64_golden.py quotes: the distance of the fp32 reference
from the float64 yardstick (tests/segloss64.py) per quantity, the near-tie census of the neighbour tables, the singular-value floor."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import segloss64 as s64  # noqa: E402

REF = os.environ.get("NVFI_REFERENCE", make_golden.REF)
ROW_STRIDE = 4
SV_FLOOR = 1e-3          # R, t are compared where sigma_min / sigma_max of S_k is above this
BAND = 1e-5              # near-tie band (relative) of the neighbour tables
BAND_CAP = 5e-3          # at most this fraction of the points may sit inside the band


def shim_pytorch3d():
    def knn_points(p1, p2, K=1, chunk=512):
        ds, ix = [], []
        for b in range(p1.shape[0]):
            db, ib = [], []
            for i0 in range(0, p1.shape[1], chunk):
                d = p1[b, i0:i0 + chunk, None, :] - p2[b, None, :, :]
                dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                v, i = torch.sort(dd, dim=1, stable=True)
                db.append(v[:, :K]); ib.append(i[:, :K])
            ds.append(torch.cat(db)); ix.append(torch.cat(ib))
        return torch.stack(ds), torch.stack(ix), None

    def knn_gather(x, idx):
        return torch.stack([x[b][idx[b]] for b in range(x.shape[0])])

    pkg, ops = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.ops")
    ops.knn_points, ops.knn_gather = knn_points, knn_gather
    pkg.ops = ops
    sys.modules["pytorch3d"], sys.modules["pytorch3d.ops"] = pkg, ops
    return knn_points


def load_reference():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_seg_loss", os.path.join(REF, "utils", "seg_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_mlp_mask(rng, pc, K, gain=4.0):
    W1, b1 = rng.standard_normal((3, 32)) * 2.0, rng.standard_normal(32)
    W2 = rng.standard_normal((32, K)) * gain / np.sqrt(32)
    z = np.tanh(pc.astype(np.float64) @ W1 + b1) @ W2
    z -= z.max(1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def two_motions(rng, pc, noise=1e-3):
    p = pc.astype(np.float64)
    Ra, ta = rot([0.2, 1.0, 0.3], 7.0), np.array([0.03, -0.01, 0.02])
    Rb, tb = rot([1.0, -0.4, 0.1], -5.0), np.array([-0.02, 0.04, 0.0])
    left = p[:, :1] < 0.05
    p2 = np.where(left, p @ Ra.T + ta, p @ Rb.T + tb) + noise * rng.standard_normal(p.shape)
    return (p2 - p).astype(np.float32)


def lattice_shell(rng, n=64, r0=0.57, r1=0.63):
    edges = np.linspace(-1.0, 1.0, n + 1)
    ax = edges[:-1, None] + (edges[1:, None] - edges[:-1, None]) * rng.random((n, 3))      # one jittered coordinate per cell and axis
    x, y, z = np.meshgrid(ax[:, 0], ax[:, 1], ax[:, 2], indexing="ij")
    p = np.stack([x, y, z], -1).reshape(-1, 3)
    r = np.linalg.norm(p, axis=1)
    return p[(r >= r0) & (r <= r1)].astype(np.float32)


def run_reference(ref, pc, flow, mask, k, radius, loss_norm):
    tp, tf = torch.from_numpy(pc)[None], torch.from_numpy(flow)[None]
    out = {}
    m = torch.from_numpy(mask)[None].clone().requires_grad_(True)
    loss, pct = ref.dynamic_loss(tp, m, tf)
    loss.backward()
    out.update(dynamic=loss.item(), pc_transformed=pct[0].detach().numpy(), g_dynamic=m.grad[0].numpy().copy())
    n_obj = mask.shape[1]
    Rr, tr = ref.fit_motion_svd_batch(tp.repeat(n_obj, 1, 1), (tp + tf).repeat(n_obj, 1, 1), torch.from_numpy(mask.T.copy()))
    out.update(R=Rr.numpy(), t=tr.numpy())
    m = torch.from_numpy(mask)[None].clone().requires_grad_(True)
    loss = ref.smooth_loss(tp, m, k=k, radius=radius, loss_norm=loss_norm)
    loss.backward()
    out.update(smooth=loss.item(), g_smooth=m.grad[0].numpy().copy())
    m = torch.from_numpy(mask)[None].clone().requires_grad_(True)
    loss = ref.entropy_loss(m)
    loss.backward()
    out.update(entropy=loss.item(), g_entropy=m.grad[0].numpy().copy())
    return out


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(np.abs(a - b).max() / (np.abs(b).max() + 1e-300), np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def main():
    knn_points = shim_pytorch3d()
    ref = load_reference()
    rng = np.random.default_rng(20240611)
    pc_l = lattice_shell(rng)
    flow_l, mask_l = two_motions(rng, pc_l), random_mlp_mask(rng, pc_l, 8)
    pc_s = ((rng.random((257, 3)) - 0.5) * 0.6).astype(np.float32)
    pc_z = ((rng.random((300, 3)) - 0.5) * 0.6).astype(np.float32)
    mask_z = random_mlp_mask(rng, pc_z, 4)
    mask_z[:, 2] = 0.0
    mask_z = (mask_z / mask_z.sum(1, keepdims=True)).astype(np.float32)
    cases = {
        "lattice_k4": (pc_l, flow_l, mask_l, 4, 0.01, 1, ROW_STRIDE),
        "lattice_k16": (pc_l, flow_l, mask_l, 16, 0.1, 2, ROW_STRIDE),
        "small": (pc_s, two_motions(rng, pc_s), random_mlp_mask(rng, pc_s, 3), 4, 0.01, 1, 1),
        "zerocol": (pc_z, two_motions(rng, pc_z), mask_z, 4, 0.01, 1, 1),
    }
    fx = {"sv_floor": np.float64(SV_FLOOR), "band": np.float64(BAND)}
    worst = {}
    for name, (pc, flow, mask, k, radius, norm, stride) in cases.items():
        N, K = mask.shape
        r = run_reference(ref, pc, flow, mask, k, radius, norm)
        with torch.no_grad():
            tp = torch.from_numpy(pc)[None]
            dist, idx, _ = knn_points(tp, tp, K=k)
            idx[dist > radius] = idx[:, :, :1].repeat(1, 1, k)[dist > radius]
        idx = idx[0].numpy()
        # the yardstick's own search, and the near-tie census of the table
        yidx, raw, d2 = s64.knn_brute(pc, k, radius)
        differ, outside = s64.idx_mismatch(pc, radius, yidx, idx, BAND)
        d64 = s64.d2_64(pc, np.arange(N)[:, None], np.maximum(raw, 0))
        d64 = np.where(raw >= 0, d64, np.inf)
        with np.errstate(invalid="ignore"):
            gap = (d64[:, k] - d64[:, k - 1]) / d64[:, k]
            tie = np.isfinite(d64[:, k]) & (d64[:, k - 1] <= radius) & (gap < BAND)
            near_r = (np.abs(d64[:, :k + 1] - radius) < BAND * radius).any(1)
        inband = int((tie | near_r).sum())
        rel_r = np.abs(d64[np.isfinite(d64)] - radius).min() / radius
        replaced = float((idx[:, 1:] == idx[:, :1]).mean())
        print(f"[{name}] N {N} K {K} k {k} radius {radius}: yardstick / shim tables differ on {differ} rows ({outside} outside the band); "
              f"points inside the {BAND:g} band {inband} ({inband / N:.2%}), smallest k/k+1 gap {np.nanmin(gap):.2e}, closest distance to the "
              f"radius {rel_r:.2e} (relative), replaced slots {replaced:.1%}")
        assert outside == 0 and differ <= BAND_CAP * N and inband <= BAND_CAP * N, name
        y = s64.segloss64(pc, flow, mask, idx, norm, 1e-5)
        ok = np.nan_to_num(y["sv"][:, 2] / y["sv"][:, 0], nan=0.0) > SV_FLOOR
        print(f"[{name}] sigma_min/sigma_max per object {np.round(y['sv'][:, 2] / y['sv'][:, 0], 4)} -> R, t compared on {int(ok.sum())} of {K}")
        assert ok.sum() >= K - 1, name
        if name == "zerocol":
            assert not ok[2] and np.array_equal(r["R"][2], np.eye(3, dtype=np.float32)) and not r["t"][2].any()
        errs = {q: abs(r[q] - y[q]) / abs(y[q]) for q in ("dynamic", "smooth", "entropy")}
        errs.update({q: relerr(r[q], y[q]) for q in ("pc_transformed", "g_dynamic", "g_smooth", "g_entropy")})
        errs["R"] = max(np.abs(r["R"][o] - y["R"][o]).max() for o in range(K) if ok[o])
        errs["t"] = max(np.abs(r["t"][o] - y["t"][o]).max() for o in range(K) if ok[o])
        print(f"[{name}] fp32 reference against the float64 yardstick: " + ", ".join(f"{q} {e:.2e}" for q, e in errs.items()))
        for q, e in errs.items():
            worst[q] = max(worst.get(q, 0.0), float(e))
        rows = np.arange(0, N, stride)
        fx[f"{name}:cfg"] = np.array([k, radius, norm], np.float64)
        fx[f"{name}:rows"] = rows.astype(np.int32)
        fx[f"{name}:sv_ok"] = ok
        shared = name == "lattice_k16"          # inputs and the dynamic / entropy outputs are lattice_k4's
        if not shared:
            fx[f"{name}:pc"], fx[f"{name}:flow"], fx[f"{name}:mask"] = pc, flow, mask
            fx[f"{name}:pc_transformed"] = r["pc_transformed"][rows].astype(np.float32)
            fx[f"{name}:g_dynamic"] = r["g_dynamic"][rows].astype(np.float32)
            fx[f"{name}:g_entropy"] = r["g_entropy"][rows].astype(np.float32)
            fx[f"{name}:R"], fx[f"{name}:t"] = r["R"].astype(np.float32), r["t"].astype(np.float32)
        fx[f"{name}:losses"] = np.array([r["dynamic"], r["smooth"], r["entropy"]], np.float64)
        fx[f"{name}:g_smooth"] = r["g_smooth"][rows].astype(np.float32)
        fx[f"{name}:idx"] = (idx if name == "lattice_k4" else idx[rows]).astype(np.int16 if N < 32768 else np.int32)
    print("worst distance of the fp32 reference from the yardstick per quantity (x 4 = the bounds of tests/test_segloss64_golden.py):")
    print("  " + ", ".join(f"{q} {e:.2e}" for q, e in worst.items()))
    path = os.path.join(HERE, "segloss.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
