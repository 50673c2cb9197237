"""Float64 restatement, with autograd, of differentiable advection (include/nvfi_hip.h: nvfi_advect_grad; TensorVMKeyframeTimeKplane.advect): the
yardstick of tests/test_advect_golden.py (against the reference's autograd through its own integrate_pos, models/tensorf_keyframe.py:575-611) and
of tests/test_gpu_advect.py (against the device).  Built from render64._vel (the gated velocity) and the step loop of flow64.schedule.  The contract:

  xk = integrate_pos(x, t, t_target): RK2 midpoint steps of at most dt_max = ts / 2 from t to t_target, the last one taking the remainder,
       x <- x - d v_g(x - d/2 v_g(x, tc), tc - d/2); v_g is gated to zero outside the box of VelocityAABB[Sur], tested on the current point and on
       the midpoint; with the surround box a step that leaves it is rejected (x stays).  t == t_target: no step.
  gx, the 12 gradients of vel_net.weight_net: those of sum(xk * g) with every discrete decision (gate, rejection) held fixed.

Like render64 / flow64, what is fixed before the net is touched stays fp32-rounded - the positions, the two times, the schedule (a scalar fp32
recurrence) - and the decisions are taken on fp32-rounded values; everything else runs in `dtype`.  dtype=float32 is "a plain fp32 implementation" of
the same statement: its distance from the float64 run is the noise floor the bounds of both test files are derived from.  Points within 4 fp32 ulp of a
gate or box face at any evaluation are reported (`edge`): there an fp32 evaluation may decide the other way."""
import numpy as np
import torch

import flow64
import render64 as r64

NET_NAMES = r64.VEL_NAMES
KEYS = ("xk", "gx") + tuple(NET_NAMES)

# The plain-fp32 noise floor of the statement: max |advect64(float32) - advect64(float64)| / max |advect64(float64)| for (xk, gx, the worst of the 12
# net tensors), measured on the CPU on the golden cases (tests/golden/make_golden_advect.py prints and records them; tests/test_advect_golden.py
# measures them again and fails when one exceeds its entry here), rounded up to two digits.  Source: that script's run on the reference, CPU, torch 2.10.
GOLDEN_FLOOR = {
    "A:c0": (0.0, 0.0, 0.0), "A:c1": (3.2e-8, 5.4e-8, 1.4e-6), "A:c2": (7.0e-8, 1.1e-7, 1.1e-6), "A:c3": (5.9e-8, 8.9e-8, 9.6e-7), "A:c4": (1.2e-7, 1.2e-7, 4.7e-7),
    "B:c0": (0.0, 0.0, 0.0), "B:c1": (2.9e-8, 4.9e-8, 9.0e-7), "B:c2": (7.1e-8, 1.1e-7, 6.0e-7), "B:c3": (1.6e-7, 2.0e-7, 4.3e-7), "B:c4": (1.6e-7, 1.9e-7, 3.3e-7),
}
ULP32 = float(np.finfo(np.float32).eps)      # no bound of the test files goes below one fp32 ulp of the tensor's scale


def golden_net(gold_dir, case):
    """the 12 reference gradients of a golden case (exact zeros for c0, which stores none)"""
    import os
    kind, name = case.split(":")
    if name == "c0":
        return None
    z = np.load(os.path.join(gold_dir, f"advect_net_{kind}{1 if name in ('c1', 'c2') else 2}.npz"))
    return {k: z[f"{case}:{k}"] for k in NET_NAMES}


def schedule(field, t, t_target):
    """[(t_curr, step_dt, t_mid), ...] of integrate_pos(x, t, t_target) in fp32 scalars: flow64.schedule's loop with the target given instead of
    t + dt (which is rounded once more) - the two agree whenever fp32(t) + fp32(dt) is exact (asserted in tests/test_advect_golden.py)"""
    t32 = torch.tensor(float(t), dtype=torch.float32)
    t1 = torch.tensor(float(t_target), dtype=torch.float32)
    dt_max = torch.ones_like(t32) * (0.5 * field.tmax / (field.K - 1) if field.K > 1 else 1)
    off, cur, steps = t32 - t1, t32.clone(), []
    while bool(off.abs() > 0):
        if len(steps) >= flow64.MAX_STEPS:
            raise ValueError(f"t={t} -> t_target={t_target} needs more than {flow64.MAX_STEPS} RK2 steps")
        d = off.sign() * torch.minimum(off.abs(), dt_max)
        steps.append((float(cur), float(d), float(cur - 0.5 * d)))
        off, cur = off - d, cur - d
    return steps


def rk2_back(P, field, x0, steps, dtype):
    """the ONE step loop of the float64 yardsticks that need more than the end point (advect64 below, alpha64.compute_alpha64): the steps
    [(t_curr, d, t_mid), ...] applied to the points x0 (N, 3, `dtype`, on any device) -> the end points and dict(n_rejected, edge, gated_all,
    n_outside) as advect64 documents them.  Differentiable where x0 / P require it."""
    device = x0.device
    lo, hi = field.lo.to(device), field.hi.to(device)
    N = x0.shape[0]
    edge = np.zeros(N, bool)
    gated_all = torch.ones(N, dtype=torch.bool, device=device)
    cur, nrej = x0, 0

    def outside(p):
        p32 = p.detach().to(torch.float32)
        return ((p32 < lo) | (p32 > hi)).any(-1)

    n_outside = int(outside(x0).sum())
    for tc, d, tm in steps:
        v1, in1 = r64._vel(P, cur, tc, field, dtype)
        pm = cur - 0.5 * d * v1
        v2, in2 = r64._vel(P, pm, tm, field, dtype)
        xc = cur - d * v2
        gated_all &= ~in1 & ~in2
        edge |= flow64._near_face(cur.cpu(), field.lo, field.hi) | flow64._near_face(pm.cpu(), field.lo, field.hi)
        if field.sur:
            rej = outside(xc)
            edge |= flow64._near_face(xc.cpu(), field.lo, field.hi)
            nrej += int((rej & ~outside(cur)).sum())          # (a point outside the gate never moves: not counted)
            xc = torch.where(rej[:, None], cur, xc)
        cur = xc
    return cur, dict(n_rejected=nrej, edge=edge, gated_all=gated_all.cpu().numpy(), n_outside=n_outside)


def advect64(field, x, t, t_target, g, dtype=torch.float64, device="cpu"):
    """dict: xk, gx (N, 3), the 12 gradients under their reference names (numpy, `dtype`), steps (the schedule), n_rejected (steps of points INSIDE
    the surround box that left it and were rejected, summed over points and steps), edge (bool per point), gated_all (bool per point: outside the
    gate at every evaluation - the point never moves and its gradient passes through unchanged), n_outside (points outside the gate at the start)"""
    x32 = torch.as_tensor(np.asarray(x, np.float32)).reshape(-1, 3)
    g32 = torch.as_tensor(np.asarray(g, np.float32)).reshape(-1, 3)
    x0 = x32.to(device=device, dtype=dtype).requires_grad_(True)
    P = {k: field.p32[k].to(device=device, dtype=dtype).requires_grad_(True) for k in NET_NAMES}
    steps = schedule(field, t, t_target)
    cur, out = rk2_back(P, field, x0, steps, dtype)
    out["steps"] = steps
    loss = (cur * g32.to(device=device, dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, [x0] + [P[k] for k in NET_NAMES], allow_unused=True)
    out["xk"] = cur.detach().cpu().numpy()
    out["gx"] = grads[0].cpu().numpy() if grads[0] is not None else g32.to(dtype).numpy()
    for k, gr in zip(NET_NAMES, grads[1:]):
        out[k] = (torch.zeros_like(P[k]) if gr is None else gr).cpu().numpy()
    return out


def floors(y32, y64):
    """(xk, gx, worst net tensor): flow64.rel_err of the float32 run against the float64 run"""
    return (flow64.rel_err(y32["xk"], y64["xk"]), flow64.rel_err(y32["gx"], y64["gx"]), max(flow64.rel_err(y32[k], y64[k]) for k in NET_NAMES))


def case_inputs(N):
    """the inputs of every test case of size N: positions that reach 5 % beyond the unit box on every side, a Gaussian upstream gradient"""
    rng = np.random.default_rng(11 + N)
    x = (rng.random((N, 3)) * 2.1 - 1.05).astype(np.float32)
    g = rng.standard_normal((N, 3)).astype(np.float32)
    return x, g
