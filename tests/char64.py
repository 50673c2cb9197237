"""Float64 restatement, with autograd, of the characteristic loss (include/nvfi_hip.h: nvfi_char_loss; reference
TensorVMKeyframeTimeKplane.characteristic_loss, models/tensorf_keyframe.py:552-573, with the semantics of its formula): the yardstick of
tests/test_charloss_golden.py (against goldens made from the reference's pieces) and of tests/test_gpu_charloss.py (against the device).

  inputs: normalised points x (N,3), the points x0 they are advected back to (GIVEN: the warp is a constant of the loss), the keyframe row k.
  t'      the normalised time of keyframe row r is 2 r / (K - 1) - 1: the time coordinate of a lookup lands ON row r
  d(x, r) = sum_c prod_i space_i(x_a, x_b)[c] time_i(x_c, t'_r)[c]      compute_densityfeature (tensorf_keyframe.py:233-272)
  a(x, r) = basis_mat (prod_i space_i time_i)                            compute_appfeature (tensorf_keyframe.py:274-310)
  loss_d  = mean_N (d(x, k) - d(x0, 0))^2        loss_a = mean_{N x app_dim} (a(x, k) - a(x0, 0))^2
  every plane lookup is bilinear F.grid_sample(align_corners=True, padding_mode="zeros"): a tap outside the plane
  contributes zero and receives no gradient.

What is fixed before the planes are touched stays fp32-rounded and is then promoted (the points, x0); everything else runs in `dtype`.
dtype=float32 is a plain fp32 implementation of the same statement.  Parameters are a dict keyed by the reference's names without the `nvfi.`
prefix (the twelve planes, logical (1,C,H,W), and basis_mat.weight)."""
import numpy as np
import torch
import torch.nn.functional as F

import render64 as r64

NAMES = r64.PLANE_NAMES + ["basis_mat.weight"]
TERMS = ("loss_d", "loss_a")


def params_from_sd(sd):
    """the 13 tensors of the loss from a state dict (numpy values; keys with or without the `nvfi.` prefix)"""
    sd = {(k[5:] if k.startswith("nvfi.") else k): v for k, v in sd.items()}
    return {n: np.ascontiguousarray(np.asarray(sd[n]), dtype=np.float32) for n in NAMES}


def snap_time(K, tmax, t):
    """(t_k, row k) of a call at time t, fp32 like the reference's tensors (tensorf_keyframe.py:554-561)"""
    t = np.float32(float(t))
    if t > 0:
        ts = np.float32(float(tmax) / (K - 1) if K > 1 else 1.0)
        q = np.rint(np.clip(t / ts, np.float32(0), np.float32(K - 1)))
        return float(q * ts), int(q)
    return float(np.float32(float(tmax)) / np.float32(K - 1)), 1


def char64(params, K, points, points0, row, dtype=torch.float64, grads=True):
    """{loss_d, loss_a (python floats), grads: {name: numpy (1,C,H,W) / (app_dim, Ca)}}"""
    P = {n: torch.from_numpy(np.asarray(params[n], np.float32)).to(dtype).requires_grad_(grads) for n in NAMES}
    x = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).reshape(-1, 3).to(dtype)
    x0 = torch.from_numpy(np.ascontiguousarray(points0, dtype=np.float32)).reshape(-1, 3).to(dtype)

    def at(q, r):
        tn = torch.full_like(q[:, :1], 2.0 * r / (K - 1) - 1.0)
        q4 = torch.cat([q, tn], 1)
        return r64._planes(P, "density", q4).sum(0), F.linear(r64._planes(P, "app", q4).T, P["basis_mat.weight"])

    d_t, a_t = at(x, int(row))
    d_0, a_0 = at(x0, 0)
    loss_d, loss_a = ((d_t - d_0) ** 2).mean(), ((a_t - a_0) ** 2).mean()
    out = dict(loss_d=float(loss_d.detach()), loss_a=float(loss_a.detach()))
    if grads:
        (loss_d + loss_a).backward()
        out["grads"] = {n: (np.zeros(P[n].shape) if P[n].grad is None else P[n].grad.numpy()) for n in NAMES}
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 where both agree exactly, inf for a non-zero error against an all-zero reference)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return 0.0 if err == 0.0 else (err / scale if scale > 0 else float("inf"))


def errors(got, ref):
    """{quantity: rel_err} over both loss terms and the 13 gradient tensors of two char64-shaped results"""
    out = {k: rel_err(got[k], ref[k]) for k in TERMS}
    for n in NAMES:
        out["grad:" + n] = rel_err(got["grads"][n], ref["grads"][n])
    return out


def outside_fraction(points0):
    p = np.asarray(points0, np.float32).reshape(-1, 3)
    return float((np.abs(p) > 1).any(-1).mean())


def clamped_texels(points0, grid, K):
    """{plane name suffix ("space.i" / "time.i"): bool (H, W)}: the texels a BORDER-CLAMPING bilinear rule would touch for the taps of the
    0-side lookups (points0, row 0) that lie outside their plane - what zero padding must leave alone"""
    p = np.asarray(points0, np.float64).reshape(-1, 3)
    out = {}
    for i in range(3):
        for kind, (ax, ay) in (("space", r64.MAT_SPACE[i]), ("time", r64.MAT_TIME[i])):
            W = grid[ax]
            H = grid[ay] if kind == "space" else K
            gx = (p[:, ax] + 1) * (W - 1) / 2
            gy = (p[:, ay] + 1) * (H - 1) / 2 if kind == "space" else np.zeros(len(p))
            m = np.zeros((H, W), bool)
            for dy in (0, 1):
                for dx in (0, 1):
                    ix, iy = np.floor(gx).astype(np.int64) + dx, np.floor(gy).astype(np.int64) + dy
                    if kind == "time" and dy:
                        continue
                    oob = (ix < 0) | (ix >= W) | (iy < 0) | (iy >= H)
                    m[np.clip(iy[oob], 0, H - 1), np.clip(ix[oob], 0, W - 1)] = True
            out[f"{kind}.{i}"] = m
    return out
