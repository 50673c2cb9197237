"""Float64 restatement, with autograd, of the 2-D mask loss of a render (include/nvfi_hip.h: nvfi_mask_loss_fwd / nvfi_mask_loss_bwd;
TensorVMKeyframeTimeKplane.mask_loss, mask_fit_backward_, render_mse_backward_(target_mask=)): the yardstick of tests/test_maskloss_golden.py (what
a lost entry or a swapped label moves, the plain-fp32 floors) and of tests/test_gpu_maskloss.py (the device).  Built from render64.sample_rays,
the back-warp of the render yardstick (render64.time_plan / render64._vel, as objects64 walks it) and maskfield64 / objects64.mask_field.  The
contract, restated:

  inputs: rays, the per-ray jitter of a training render (None: an eval render), t, the MaskField's ten tensors, a target, and a GIVEN fp32 weight
          map (R, S) - the render's own output.
  M_r   the samples of ray r with weight > float32(rayMarch_weight_thres) (an fp32 comparison on the given map), or the mask given
  x_j   the sample's position warped back to the keyframe time: RK2 steps of the gated velocity net, the surround rule of the render
  m_jk  = softmax(MaskField(x_j))_k
  q[r][k] = sum_{j in M_r} w_j m_jk
  target: int labels (R): [0, K) one-hot, K all zero (background), anything else ignores the ray; float rows (R, K): a non-finite entry ignores the ray
  n     = the rays that are not ignored
  loss  = 1 / (2 n K) sum_valid sum_k (q - y)^2 ("l2"),  -(1 / n) sum_valid sum_k y log(q + eps) ("ce");  n == 0: 0
  g_weights and the ten MaskField gradients: those of `loss` with the mask, the positions and n held fixed.  The positions carry no gradient.

What is fixed before a net is touched stays fp32-rounded - sample positions, times, the schedule, the weights, aabb, the MaskField's values, the
target, eps - and decisions are taken on fp32-rounded values; everything else runs in `dtype`.  dtype=float32 is "a plain fp32 implementation"
of the same statement: its distance from the float64 run is the noise floor the bounds of both test files are derived from.  `margin` reports
maskfield64.margin() per entry: how many fp32 rounding bounds the nearest hidden pre-activation of the MaskField stays away from its ReLU kink."""
import numpy as np
import torch

import maskfield64 as m64
import render64 as r64
from objects64 import mask_field

GRAD_KEYS = m64.GRAD_KEYS
KEYS = ("mask_map", "loss", "g_weights") + tuple(GRAD_KEYS)
ULP32 = float(np.finfo(np.float32).eps)

# Bounds (bounds()): never from the device.  Per tensor, relative to the tensor's max: max(3 x d32, floor), d32 the float32 evaluation's distance
# from the float64 one on the SAME case (same weights, same list), 3 the project's headroom for another summation order (render64, raydist64,
# maskfield64).  The floors keep a tensor whose own fp32 figure happens to be tiny from getting a bound below what another order of the same
# sums may cost:
#   mask_map   q <= 1 is a sum of <= S products w m: MASK_FLOOR of maskfield64 (4 ulp of 1.0: expf, the division, the 128-term logit sum) on the
#              map's scale
#   loss       the mean of R K terms in fp64 of fp32 terms: one fp32 rounding of the term + that of q, and for ce the logf (2 ulp): 8 ulp
#   g_weights  a K-term dot product of g_q (2 roundings) and m (MASK_FLOOR): 3 x MASK_FLOOR
#   the ten    maskfield64.FLOOR_G = 3 x the largest fp32 figure of MaskField's own matrix, measured on the CPU there
# tests/test_maskloss_golden.py measures d32 on the CPU cases again and fails when one exceeds CPU_D32_MAX.
MAP_FLOOR = m64.MASK_FLOOR
LOSS_FLOOR = 8 * ULP32
GW_FLOOR = 3 * m64.MASK_FLOOR
FLOOR_G = m64.FLOOR_G
# largest d32 over the cases of tests/test_maskloss_golden.py (fields A and B, K = 2, 8, 17, 32, both kinds, labels and soft), CPU, 4 threads:
# (mask_map, loss, g_weights, worst of the ten) measured 3.8e-7, 1.5e-7, 4.9e-7, 7.4e-7; stated with a third of headroom for another BLAS
# blocking of torch's fp32 matrix sums
CPU_D32_MAX = (5.0e-7, 2.0e-7, 7.0e-7, 1.0e-6)


def targets(target, R, K):
    """(y (R, K) float32 with ignored rows zeroed, ok (R) bool) of int labels (R) or float rows (R, K)"""
    tg = np.asarray(target)
    if tg.dtype.kind in "iu":
        lab = tg.reshape(R).astype(np.int64)
        ok = (lab >= 0) & (lab <= K)
        y = np.zeros((R, K), np.float32)
        hot = ok & (lab < K)
        y[np.nonzero(hot)[0], lab[hot]] = 1.0
        return y, ok
    y = tg.astype(np.float32).reshape(R, K).copy()
    ok = np.isfinite(y).all(1)
    y[~ok] = 0.0
    return y, ok


def warp_masked(field, smp, mask, t, transfer=False, dtype=torch.float64, device="cpu"):
    """the masked samples' positions at the keyframe time, (M, 3) in `dtype`, list order (ray-major): objects64's walk of the render's back-warp"""
    plan = r64.time_plan(field, t, transfer)
    P = {k: field.p32[k].to(device=device, dtype=dtype) for k in r64.VEL_NAMES}
    x = smp["xn"][mask].to(device=device, dtype=dtype)
    with torch.no_grad():
        for tc, dt, tm in plan["steps"]:
            v1, _ = r64._vel(P, x, tc, field, dtype)
            v2, _ = r64._vel(P, x - 0.5 * dt * v1, tm, field, dtype)
            xc = x - dt * v2
            if field.sur:
                c32 = xc.to(torch.float32)
                out = ((c32 < field.lo.to(device)) | (c32 > field.hi.to(device))).any(-1)
                xc = torch.where(out[:, None], x, xc)
            x = xc
    return x


def maskloss64(field, mparams, rays_o, rays_d, t, weights, jitter, target, kind="ce", eps=1e-5, mask=None, points=None, transfer=False,
               dtype=torch.float64, device="cpu", want_margin=True):
    """dict: mask_map (R, K), loss, n, g_weights (R, S), the ten gradients under GRAD_KEYS (numpy, `dtype`), mask (R, S), M, idx ((M, 2) ray,
    sample - the device's list order), x (M, 3) the positions used, margin (M) maskfield64.margin per entry.  points: (M, 3) fp32 positions to use
    instead of the yardstick's own warp (the device's export)."""
    smp = r64.sample_rays(field, rays_o, rays_d, jitter)
    R, S = smp["valid"].shape
    K = int(np.asarray(mparams[8]).shape[0])
    w32 = torch.as_tensor(np.asarray(weights, np.float32)).reshape(R, S)
    if mask is None:
        mask = w32 > torch.tensor(field.thres, dtype=torch.float32)
    mask = torch.as_tensor(np.asarray(mask, bool)).reshape(R, S)
    idx = mask.nonzero()
    ray = idx[:, 0].to(device)
    if points is None:
        x = warp_masked(field, smp, mask, t, transfer, dtype, device)
    else:
        x = torch.as_tensor(np.asarray(points, np.float32)).to(device=device, dtype=dtype)
    w = w32[mask].to(device=device, dtype=dtype).requires_grad_(True)
    ps = [torch.as_tensor(np.asarray(p, np.float32)).to(device=device, dtype=dtype).requires_grad_(True) for p in mparams]
    m = mask_field(ps, x, dtype)
    q = torch.zeros(R, K, dtype=dtype, device=device).index_add(0, ray, w[:, None] * m)
    y32, ok = targets(target, R, K)
    y = torch.as_tensor(y32).to(device=device, dtype=dtype)
    okt = torch.as_tensor(ok).to(device)
    n = int(ok.sum())
    if n == 0:
        loss = q.sum() * 0
    elif kind == "l2":
        loss = (((q - y) ** 2) * okt[:, None].to(dtype)).sum() / (2 * n * K)
    elif kind == "ce":
        e = torch.tensor(float(np.float32(eps)), dtype=dtype, device=device)
        terms = torch.where(y != 0, -y * torch.log(q + e), torch.zeros_like(q))      # (a background ray adds nothing, but counts in n)
        loss = (terms * okt[:, None].to(dtype)).sum() / n
    else:
        raise ValueError(kind)
    grads = torch.autograd.grad(loss, [w] + ps, allow_unused=True)
    gw = torch.zeros(R, S, dtype=dtype)
    if grads[0] is not None:
        gw[mask] = grads[0].cpu()
    out = dict(mask_map=q.detach().cpu().numpy(), loss=float(loss.detach()), n=n, g_weights=gw.numpy(), mask=mask.numpy(), M=int(mask.sum()),
               idx=idx.numpy(), x=x.detach().cpu().numpy(), ok=ok, weights32=w32.numpy())
    for k, p, gr in zip(GRAD_KEYS, ps, grads[1:]):
        out[k] = (torch.zeros_like(p) if gr is None else gr).cpu().numpy()
    if want_margin:
        out["margin"] = m64.margin(mparams, out["x"].astype(np.float32)) if out["M"] else np.zeros(0)
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 for an all-zero reference that is matched exactly)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    s = np.abs(ref).max() if ref.size else 0.0
    d = np.abs(got - ref).max() if ref.size else 0.0
    return 0.0 if d == 0 else (float("inf") if s == 0 else float(d / s))


def d32(y32, y64):
    """(mask_map, loss, g_weights, worst of the ten): the float32 run against the float64 run, relative to the tensor's max"""
    ls = abs(y32["loss"] - y64["loss"]) / abs(y64["loss"]) if y64["loss"] != 0 else (0.0 if y32["loss"] == 0 else float("inf"))
    return (rel_err(y32["mask_map"], y64["mask_map"]), ls, rel_err(y32["g_weights"], y64["g_weights"]),
            max(rel_err(y32[k], y64[k]) for k in GRAD_KEYS))


def bounds(y32, y64):
    """(mask_map, loss, g_weights, the ten): max(3 x the case's own float32 distance, the floor)"""
    d = d32(y32, y64)
    return tuple(max(3 * v, f) for v, f in zip(d, (MAP_FLOOR, LOSS_FLOOR, GW_FLOOR, FLOOR_G)))


def entry_flips(mparams, y64, target, kind, eps, limit=1.0):
    """maskfield64.gate_flips for the masked entries of a yardstick result: x the entries' positions, g the entries' g_mask = w_j g_q[ray(j)] in
    float64 - [((entry, layer, unit, margin), {gradient key: change})] for maskfield64.admit_flips"""
    R, K = y64["mask_map"].shape
    y, ok = targets(target, R, K)
    q = y64["mask_map"]
    n = max(int(ok.sum()), 1)
    if kind == "l2":
        gq = (q - y) / (n * K)
    else:
        gq = np.where(y != 0, -y / (q + float(np.float32(eps))) / n, 0.0)
    gq = gq * ok[:, None]
    ray, smp = y64["idx"][:, 0], y64["idx"][:, 1]
    w = np.asarray(y64["weights32"], np.float64)[ray, smp]
    g = w[:, None] * gq[ray]
    return m64.gate_flips(mparams, y64["x"].astype(np.float32), g, limit)


# ---------------------------------------------------------------------------------------------------------------- the rays of the device tests
# The render's points cannot be redrawn, so the per-ray jitter of every case of tests/test_gpu_maskloss.py is drawn from a seed under which the
# CPU float32 run of the yardstick alone (render64's own fp32 weights) keeps the share of masked entries within one rounding bound of a MaskField
# ReLU kink under maskfield64.KINK_CAP - for the small cases: no such entry at all.  tests/test_maskloss_golden.py checks the table on the CPU.
GPU_SHAPES = (1, 2, 33, 65, 257)
# (the first seed from 11 + R on whose share is at most half the cap: the device's own weights move the list a little.  CPU figures: A 0 of 25, 0 of
# 24, 9 of 882, 20 of 1 719, 87 of 7 779 entries; B 0 of 28, 0 of 27, 6 of 842, 17 of 1 679, 87 of 7 174)
JITTER_SEED = {("A", 1): 12, ("A", 2): 13, ("A", 33): 46, ("A", 65): 76, ("A", 257): 269,
               ("B", 1): 12, ("B", 2): 14, ("B", 33): 45, ("B", 65): 78, ("B", 257): 269}


def gpu_rays(gold, kind, R, seed=None):
    """(rays_o, rays_d, jitter) of the case of R rays: golden rays 100 .. 100 + R of the hot-path fixture (ray 100 hits the object); from R = 2 on
    the last ray looks away from the box (nothing valid, nothing masked)"""
    idx = [i % 256 for i in range(100, 100 + R)]
    o, d = gold[f"{kind}:rays_o"][idx].copy(), gold[f"{kind}:rays_d"][idx].copy()
    if R >= 2:
        d[-1] = -d[-1]
    jit = np.random.default_rng(JITTER_SEED[kind, R] if seed is None else seed).random(R).astype(np.float32)
    return o, d, jit


def kink_share(field, o, d, jit, t):
    """(share of masked entries with margin < 1, their number, M) of the CPU float32 run of the yardstick on render64's own fp32 training weights"""
    w = r64.render64(field, o, d, t, jit, True, grads=False, dtype=torch.float32)["weight"]
    y = maskloss64(field, m64.params_for(8), o, d, t, w, jit, np.zeros(len(o), np.int32), dtype=torch.float32)
    low = int((y["margin"] < 1.0).sum())
    return (low / y["M"] if y["M"] else 0.0), low, y["M"]
