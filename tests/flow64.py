"""Float64 restatement of the flow branch of an eval-mode render (include/nvfi_hip.h: nvfi_render_flow; the reference has no such call - its
pieces are the reference's own VelocityAABB[Sur].forward, models/velocity_field.py:21-51, and integrate_pos, models/tensorf_keyframe.py:575-611):
the yardstick of tests/test_flow_golden.py (against maps composited from the reference's field.vel / field.integrate_pos) and of
tests/test_gpu_flow.py (against the device).  The contract, restated:

  inputs: rays, t, dt, a camera (pose 3x4, H, W, focal) or None, and a GIVEN fp32 weight map (R, S) - the render's own output.
  M_r   the samples of ray r with weight > float32(rayMarch_weight_thres) (an fp32 comparison on the given map)
  x_j   the UN-warped normalised sample position at time t: render64.sample_rays without jitter, fp32
  s     aabbSize / 2 per axis
  vel_map[r]  = sum_{j in M_r} w_j s * v_g(x_j, t)                  v_g the gated velocity at the raw time t
  flow_map[r] = sum_{j in M_r} w_j s * (Phi(x_j) - x_j)             Phi(x) = integrate_pos(x, t, t + dt): RK2 midpoint steps of at most dt_max,
        the last one takes the remainder, x <- x + step * v_g(x + step/2 * v_g(x, tc), tc + step/2) (integrate_pos subtracts its own dt = -step),
        the gate on the current point, and with the surround box a step that leaves it is rejected.  dt == 0: no step, exact zeros
  flow2d[r]   = sum_{j in M_r} w_j (pi(P'_j) - pi(P_j))             P = aabb0 + (x + 1) s; c = R^T (P - o_cam); pi = (W/2 + focal c_x / -c_z,
        H/2 - focal c_y / -c_z); a sample whose displaced point has -c_z < 1e-3 contributes nothing

Like render64, what is fixed before the field is touched stays fp32-rounded - positions, t, t + dt, the RK2 schedule (a scalar fp32 recurrence),
the weights, aabb, the pose - and the discrete decisions (mask, gate, step rejection) are taken on fp32-rounded values; everything else runs in
`dtype`.  dtype=float32 is "a plain fp32 implementation" of the same statement: its distance from the float64 run is the noise floor the bounds of
both test files are derived from.  Samples whose gate or rejection decision lies within 4 fp32 ulp of a face are reported (`edge_samples`,
`edge_rays`): there an fp32 evaluation may decide the other way and the sample's displacement jumps."""
import numpy as np
import torch

import render64 as r64

# The plain-fp32 noise floor of the statement below: max |flow64(float32) - flow64(float64)| / max |flow64(float64)| per map (vel_map, flow_map,
# flow2d), measured on the CPU on the golden cases (tests/golden/make_golden_flow.py prints and records them; tests/test_flow_golden.py measures
# them again and fails when one exceeds its entry here), rounded up to two digits.  Source: that script's run on the reference, CPU, torch 2.10.
GOLDEN_FLOOR = {
    "A:c1": (2.8e-7, 2.5e-7, 2.7e-6), "A:c2": (2.8e-7, 1.8e-7, 5.2e-7), "A:c3": (2.4e-7, 2.8e-7, 1.1e-6), "A:c4": (2.5e-7, 2.5e-7, 6.9e-7),
    "A:c5": (2.1e-7, 3.0e-7, 2.5e-6), "A:c6": (2.8e-7, 0.0, 0.0),
    "B:c1": (3.2e-7, 7.4e-7, 9.6e-6), "B:c2": (3.2e-7, 4.1e-7, 1.6e-6), "B:c3": (2.7e-7, 4.5e-7, 3.6e-6), "B:c4": (3.9e-7, 2.5e-7, 6.1e-7),
    "B:c5": (3.3e-7, 5.7e-7, 6.9e-6), "B:c6": (3.2e-7, 0.0, 0.0), "B:c7": (3.2e-7, 4.4e-7, 1.1e-6),
}
MAP_KEYS = ("vel_map", "flow_map", "flow2d")
MAX_STEPS = 64       # the library's step limit (MAX_RK_STEPS): more is refused, not truncated


def schedule(field, t, dt):
    """[(t_curr, step_dt, t_mid), ...] of integrate_pos(x, t, t + dt) in fp32 scalars; step_dt has integrate_pos' sign (x <- x - step_dt v)"""
    t32 = torch.tensor(float(t), dtype=torch.float32)
    t1 = t32 + torch.tensor(float(dt), dtype=torch.float32)
    dt_max = torch.ones_like(t32) * (0.5 * field.tmax / (field.K - 1) if field.K > 1 else 1)
    off, cur, steps = t32 - t1, t32.clone(), []
    while bool(off.abs() > 0):
        if len(steps) >= MAX_STEPS:
            raise ValueError(f"dt={dt} needs more than {MAX_STEPS} RK2 steps")
        d = off.sign() * torch.minimum(off.abs(), dt_max)
        steps.append((float(cur), float(d), float(cur - 0.5 * d)))
        off, cur = off - d, cur - d
    return steps


def _near_face(x, lo, hi, n_ulp=4):
    """bool per point: some coordinate of the fp32 rounding of x within n_ulp fp32 ulp of a face of the box [lo, hi]"""
    x32 = x.detach().to(torch.float32).numpy()
    out = np.zeros(len(x32), bool)
    for face in (lo.numpy(), hi.numpy()):
        tol = n_ulp * np.spacing(np.abs(face).astype(np.float32))
        out |= (np.abs(x32 - face) <= tol).any(-1)
    return out


def project(P, pose, focal):
    """pixel offsets from the principal point (u - W/2, v - H/2) and depth -c_z of world points P (n, 3)"""
    q = P - pose[:, 3]
    c = q @ pose[:, :3]                    # R^T q
    depth = -c[:, 2]
    return focal * c[:, 0] / depth, -(focal * c[:, 1] / depth), depth


def flow64(field, rays_o, rays_d, t, dt, weights, camera=None, dtype=torch.float64, want=("vel", "flow", "flow2d")):
    """the three maps (numpy, `dtype`) + `mask` (R, S), `M`, `edge_samples` ((n, 2) ray, sample), `edge_rays`, `n_rejected` (steps of points INSIDE the surround box that
    left it and were rejected, summed over samples and steps), `steps`"""
    smp = r64.sample_rays(field, rays_o, rays_d, None)
    R, S = smp["valid"].shape
    w32 = torch.as_tensor(np.asarray(weights, np.float32)).reshape(R, S)
    mask = w32 > torch.tensor(field.thres, dtype=torch.float32)
    idx = mask.nonzero()                              # ray-major, sample-minor: the device's list order
    ray = idx[:, 0]
    x0 = smp["xn"][mask].to(dtype)
    w = w32[mask].to(dtype)
    P = {k: v.to(dtype) for k, v in field.p32.items() if k in r64.VEL_NAMES}
    half = ((field.aabb[1] - field.aabb[0]) / 2).to(dtype)
    t32 = float(np.float32(float(t)))
    edge = np.zeros(len(x0), bool)
    out = dict(mask=mask.numpy(), M=int(mask.sum()))

    def seg(val):
        return torch.zeros(R, val.shape[1], dtype=dtype).index_add(0, ray, w[:, None] * val).numpy()

    with torch.no_grad():
        if "vel" in want:
            v, _ = r64._vel(P, x0, t32, field, dtype)
            edge |= _near_face(x0, field.lo, field.hi)
            out["vel_map"] = seg(half * v)
        steps = schedule(field, t, dt)
        x, nrej = x0, 0
        if "flow" in want or "flow2d" in want:
            for tc, d, tm in steps:
                v1, _ = r64._vel(P, x, tc, field, dtype)
                pm = x - 0.5 * d * v1
                v2, _ = r64._vel(P, pm, tm, field, dtype)
                xc = x - d * v2
                edge |= _near_face(x, field.lo, field.hi) | _near_face(pm, field.lo, field.hi)
                if field.sur:
                    c32 = xc.to(torch.float32)
                    rej = ((c32 < field.lo) | (c32 > field.hi)).any(-1)
                    edge |= _near_face(xc, field.lo, field.hi)
                    x32 = x.to(torch.float32)
                    nrej += int((rej & ~((x32 < field.lo) | (x32 > field.hi)).any(-1)).sum())     # (a point outside the gate never moves: not counted)
                    xc = torch.where(rej[:, None], x, xc)
                x = xc
            out["flow_map"] = seg(half * (x - x0))
        if "flow2d" in want and camera is not None:
            pose, H, W, focal = camera
            pose = torch.as_tensor(np.asarray(pose, np.float32))[:3, :4].to(dtype)
            a0 = field.aabb[0].to(dtype)
            u0, v0, _ = project(a0 + (x0 + 1) * half, pose, float(np.float32(focal)))
            u1, v1_, z1 = project(a0 + (x + 1) * half, pose, float(np.float32(focal)))
            keep = ~(z1.to(torch.float32) < np.float32(1e-3))
            d2 = torch.stack([u1 - u0, v1_ - v0], 1)
            out["flow2d"] = seg(torch.where(keep[:, None], d2, torch.zeros_like(d2)))
    out["edge_samples"] = idx.numpy()[edge]
    out["edge_rays"] = np.unique(out["edge_samples"][:, 0])
    out["n_rejected"], out["steps"] = nrej, steps
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 for an all-zero reference that is matched exactly)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    return 0.0 if err == 0.0 else float(err / scale) if scale > 0 else float("inf")
