"""Float64 restatement, with autograd, of the optical-flow loss of a training render (include/nvfi_hip.h: nvfi_flow_loss_fwd / nvfi_flow_loss_bwd;
TensorVMKeyframeTimeKplane.flow_loss): the yardstick of tests/test_flowloss_golden.py (against the reference's integrate_pos under autograd) and of
tests/test_gpu_flowloss.py (against the device).  Built from flow64.project, the step loop of advect64.schedule / advect64.rk2_back and
render64.sample_rays.  The contract, restated:

  inputs: rays, the per-ray jitter of the training render, t, dt, a camera (pose 3x4, H, W, focal), a target flow (R, 2), an optional valid mask,
          and a GIVEN fp32 weight map (R, S) - the render's own output.
  M_r   the samples of ray r with weight > float32(rayMarch_weight_thres) (an fp32 comparison on the given map), or the mask given
  z_j   the sample depth of the training render: t_min + step (j + u_r), fp32;  x_j = normalize_coord(o_r + d_r z_j), fp32
  Phi   integrate_pos(x, t, t + dt) on the uniform schedule, every gate / rejection rule of advect64
  flow2d[r] = sum_{j in M_r} w_j (pi(P'_j) - pi(P_j)); a sample whose displaced point has -c_z < 1e-3 contributes nothing
  valid ray: valid[r] != 0 and a finite target; n their number; e = flow2d - target
  loss  = (1 / (2 n)) sum_valid sum_c rho(e_rc), rho(e) = e^2 ("l2") or torch's huber element ("huber"); n == 0: 0
  g_weights, the 12 gradients of vel_net.weight_net: those of `loss` with every discrete decision (mask, gate, rejection, guard, valid) held fixed.

Like flow64 / advect64, what is fixed before the net is touched stays fp32-rounded - positions, the times, the schedule, the weights, aabb, the
pose, the target - and decisions are taken on fp32-rounded values; everything else runs in `dtype`.  dtype=float32 is "a plain fp32
implementation" of the same statement: its distance from the float64 run is the noise floor the bounds of both test files are derived from.
Entries within 4 fp32 ulp of a gate face, of a box face or of the -c_z = 1e-3 guard are reported (`edge`)."""
import numpy as np
import torch
import torch.nn.functional as F

import advect64 as a64
import flow64
import render64 as r64

NET_NAMES = r64.VEL_NAMES
KEYS = ("flow2d", "loss", "g_weights") + tuple(NET_NAMES)
GUARD = float(np.float32(1e-3))
ULP32 = float(np.finfo(np.float32).eps)

# The plain-fp32 noise floor of the statement: max |flowloss64(float32) - flowloss64(float64)| / max |flowloss64(float64)| for (flow2d, loss,
# g_weights, the worst of the 12 net tensors), measured on the CPU on the golden cases (tests/golden/make_golden_flowloss.py prints and records
# them; tests/test_flowloss_golden.py measures them again and fails when one exceeds its entry here), rounded up to two digits.
# Source: that script's run on the reference, CPU, torch 2.10; the net column is the largest of runs with 1, 2, 4, 8 and 16 threads (the order of
# torch's fp32 matrix sums follows the thread count: 2.2e-7 .. 2.8e-7 for A:c4).  c6 projects with a camera inside the box: samples a few millimetres in front of its
# plane are magnified to 4e5 pixels, and so is their rounding.
GOLDEN_FLOOR = {
    "A:c0": (0.0, 2.4e-8, 0.0, 0.0), "A:c1": (2.0e-6, 8.2e-8, 3.3e-6, 3.3e-7), "A:c2": (5.7e-7, 3.0e-8, 1.2e-6, 2.1e-7), "A:c3": (2.0e-6, 5.1e-8, 7.1e-6, 3.8e-7),
    "A:c4": (2.0e-6, 9.5e-8, 3.2e-6, 2.8e-7), "A:c5": (2.0e-6, 0.0, 0.0, 0.0), "A:c6": (1.6e-4, 2.0e-4, 3.2e-4, 1.5e-4),
    "B:c0": (0.0, 5.7e-8, 0.0, 0.0), "B:c1": (7.4e-6, 7.2e-7, 2.1e-5, 3.8e-7), "B:c2": (2.2e-6, 2.1e-7, 5.0e-6, 4.0e-7), "B:c3": (7.4e-6, 6.8e-7, 2.5e-5, 5.3e-7),
    "B:c4": (7.4e-6, 7.7e-7, 2.3e-5, 3.5e-7), "B:c5": (7.4e-6, 0.0, 0.0, 0.0), "B:c6": (6.0e-4, 1.1e-3, 1.2e-3, 8.2e-5),
}


def golden_net(gold_dir, case):
    """the 12 reference gradients of a golden case (None for c0 and c5, whose gradients are exact zeros and are not stored)"""
    import os
    kind, name = case.split(":")
    if name in ("c0", "c5"):
        return None
    z = np.load(os.path.join(gold_dir, f"flowloss_net_{kind}{1 if name in ('c1', 'c2', 'c3') else 2}.npz"))
    return {k: z[f"{case}:{k}"] for k in NET_NAMES}


def golden_case(z, case):
    """the inputs of a golden case from flowloss.npz: (rays_o, rays_d, jitter, weight, camera, target, valid, dt, kind, delta)"""
    kind, name = case.split(":")
    p = kind + ":"
    cam = (z[p + ("pose_in" if name == "c6" else "pose")], int(z[p + "H"]), int(z[p + "W"]), float(z[p + "focal"]))
    R = len(z[p + "rays_o"])
    target = z[p + ("target4" if name == "c4" else "target")]
    valid = z[p + "valid4"] if name == "c4" else np.zeros(R, np.uint8) if name == "c5" else np.ones(R, np.uint8)
    return (z[p + "rays_o"], z[p + "rays_d"], z[p + "u"].reshape(-1), z[p + "weight"], cam, target, valid, float(z[case + ":dt"]), str(z[case + ":kind"]),
            float(z[case + ":delta"]))


def flowloss64(field, rays_o, rays_d, t, dt, weights, jitter, camera, target, valid=None, kind="l2", delta=1.0, mask=None,
               dtype=torch.float64, device="cpu"):
    """dict: flow2d (R, 2), loss, n, g_weights (R, S), the 12 gradients under their reference names (numpy, `dtype`), mask (R, S), M, idx ((M, 2)
    ray, sample - the device's list order), edge (bool per entry), n_guard (entries behind the guard), n_rejected, steps"""
    smp = r64.sample_rays(field, rays_o, rays_d, jitter)
    R, S = smp["valid"].shape
    w32 = torch.as_tensor(np.asarray(weights, np.float32)).reshape(R, S)
    if mask is None:
        mask = w32 > torch.tensor(field.thres, dtype=torch.float32)
    mask = torch.as_tensor(np.asarray(mask, bool)).reshape(R, S)
    idx = mask.nonzero()
    ray = idx[:, 0].to(device)
    x0 = smp["xn"][mask].to(device=device, dtype=dtype)
    w = w32[mask].to(device=device, dtype=dtype).requires_grad_(True)
    P = {k: field.p32[k].to(device=device, dtype=dtype).requires_grad_(True) for k in NET_NAMES}
    t32 = np.float32(float(t))
    t1 = np.float32(t32 + np.float32(float(dt)))
    steps = a64.schedule(field, float(t32), float(t1))
    x1, info = a64.rk2_back(P, field, x0, steps, dtype)
    pose, H, W, focal = camera
    pose = torch.as_tensor(np.asarray(pose, np.float32))[:3, :4].to(device=device, dtype=dtype)
    focal = float(np.float32(focal))
    half = ((field.aabb[1] - field.aabb[0]) / 2).to(device=device, dtype=dtype)
    a0 = field.aabb[0].to(device=device, dtype=dtype)
    u0, v0, _ = flow64.project(a0 + (x0 + 1) * half, pose, focal)
    u1, v1, z1 = flow64.project(a0 + (x1 + 1) * half, pose, focal)
    z32 = z1.detach().to(torch.float32)
    keep = ~(z32 < GUARD)
    d2 = torch.stack([u1 - u0, v1 - v0], 1)
    d2 = torch.where(keep[:, None], d2, torch.zeros_like(d2))
    flow2d = torch.zeros(R, 2, dtype=dtype, device=device).index_add(0, ray, w[:, None] * d2)
    tg32 = torch.as_tensor(np.asarray(target, np.float32)).reshape(R, 2)
    ok = torch.isfinite(tg32).all(-1)
    if valid is not None:
        ok = ok & (torch.as_tensor(np.asarray(valid)).reshape(R) != 0)
    ok = ok.to(device)
    tg = torch.where(ok[:, None], tg32.to(device), torch.zeros(1, device=device)).to(dtype)
    e = flow2d - tg
    if kind == "l2":
        rho = e * e
    elif kind == "huber":
        rho = F.huber_loss(e, torch.zeros_like(e), reduction="none", delta=float(np.float32(delta)))
    else:
        raise ValueError(kind)
    n = int(ok.sum())
    loss = (rho * ok[:, None].to(dtype)).sum() / (2 * n) if n > 0 else flow2d.sum() * 0
    grads = torch.autograd.grad(loss, [w] + [P[k] for k in NET_NAMES], allow_unused=True)
    gw = torch.zeros(R, S, dtype=dtype)
    if grads[0] is not None:
        gw[mask] = grads[0].cpu()
    out = dict(flow2d=flow2d.detach().cpu().numpy(), loss=float(loss.detach()), n=n, g_weights=gw.numpy(), mask=mask.numpy(), M=int(mask.sum()), idx=idx.numpy(),
               steps=steps, n_rejected=info["n_rejected"], n_guard=int((~keep).sum()))
    edge = np.asarray(info["edge"], bool).copy()
    edge |= np.abs(z32.cpu().numpy() - np.float32(GUARD)) <= 4 * np.spacing(np.float32(GUARD))
    edge |= flow64._near_face(x0.cpu(), torch.full((3,), -1.0), torch.full((3,), 1.0))        # a box face in normalised coordinates
    out["edge"] = edge
    for k, gr in zip(NET_NAMES, grads[1:]):
        out[k] = (torch.zeros_like(P[k]) if gr is None else gr).cpu().numpy()
    return out


def floors(y32, y64):
    """(flow2d, loss, g_weights, worst net tensor): the float32 run against the float64 run, relative to the tensor's max"""
    ls = abs(y32["loss"] - y64["loss"]) / abs(y64["loss"]) if y64["loss"] != 0 else (0.0 if y32["loss"] == 0 else float("inf"))
    return (flow64.rel_err(y32["flow2d"], y64["flow2d"]), ls, flow64.rel_err(y32["g_weights"], y64["g_weights"]),
            max(flow64.rel_err(y32[k], y64[k]) for k in NET_NAMES))


def epe(flow2d, gt, valid=None):
    """mean end-point error |flow2d - gt|_2 over the valid pixels with a finite target (float64)"""
    f, g = np.asarray(flow2d, np.float64).reshape(-1, 2), np.asarray(gt, np.float64).reshape(-1, 2)
    ok = np.isfinite(g).all(-1)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    return float(np.linalg.norm(f[ok] - g[ok], axis=-1).mean()) if ok.any() else float("nan")

