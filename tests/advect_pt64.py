"""Float64 restatement, with autograd, of differentiable advection with PER-POINT times (include/nvfi_hip_advect_pt.h: nvfi_advect_grad_pt;
TensorVMKeyframeTimeKplane.advect_pt): the yardstick of tests/test_advect_pt_golden.py (against the reference's autograd through its own
integrate_pos on (N,1) time tensors) and of tests/test_gpu_advect_pt.py (against the device).  Built on advect64.rk2_back - the one step loop of
the float64 yardsticks - and through it on render64._vel, which takes a scalar time: the points are grouped by their distinct fp32 pair
(t_i, t_target_i), every group walks its own advect64.schedule on ONE shared set of leaves (the positions, the 12 tensors of the net), and the
loss sum(xk * g) is differentiated once.  The contract is advect64's, point by point; the times get no gradient.

Defining property (asserted in tests/test_advect_pt_golden.py): advect_pt64 equals advect64.advect64 applied per distinct (t, t_target) group,
xk and gx scattered back to the points' places and the net gradients summed over the groups - to 1e-12 of each tensor's max in float64."""
import numpy as np
import torch

import advect64 as a64

NET_NAMES = a64.NET_NAMES
KEYS = a64.KEYS


def as_times(v, N):
    """a scalar or N values -> (N,) float32, the rounding every implementation starts from"""
    v = np.asarray(v, np.float64).reshape(-1)
    return np.broadcast_to(v.astype(np.float32), (N,)).copy()


def groups_of(t, t_target):
    """[(t, t_target, index array)] of the distinct fp32 pairs, in order of first appearance"""
    pairs = np.stack([t, t_target], 1)
    uniq, first, inv = np.unique(pairs, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    return [(float(uniq[k, 0]), float(uniq[k, 1]), np.nonzero(inv == k)[0]) for k in np.argsort(first)]


def advect_pt64(field, x, t, t_target, g, dtype=torch.float64, device="cpu"):
    """dict: xk, gx (N, 3), the 12 gradients under their reference names (numpy, `dtype`), steps (N ints: RK2 steps per point), groups (the number of
    distinct time pairs), and advect64's reports: n_rejected (summed over points and steps), edge / gated_all (bool per point; a point that takes
    no step is gated_all by definition: it never moves and its gradient passes through), n_outside (points outside the gate at the start)"""
    x32 = torch.as_tensor(np.asarray(x, np.float32)).reshape(-1, 3)
    g32 = torch.as_tensor(np.asarray(g, np.float32)).reshape(-1, 3)
    N = x32.shape[0]
    tt, t1 = as_times(t, N), as_times(t_target, N)
    x0 = x32.to(device=device, dtype=dtype).requires_grad_(True)
    P = {k: field.p32[k].to(device=device, dtype=dtype).requires_grad_(True) for k in NET_NAMES}
    groups = groups_of(tt, t1)
    cur = x0 * 1.0
    out = dict(steps=np.zeros(N, np.int64), n_rejected=0, edge=np.zeros(N, bool), gated_all=np.ones(N, bool), n_outside=0, groups=len(groups))
    for ta, tb, idx in groups:
        steps = a64.schedule(field, ta, tb)
        ix = torch.as_tensor(idx, device=device)
        end, rep = a64.rk2_back(P, field, x0[ix], steps, dtype)
        cur = cur.index_put((ix,), end)
        out["steps"][idx] = len(steps)
        out["n_rejected"] += rep["n_rejected"]
        out["n_outside"] += rep["n_outside"]
        out["edge"][idx] = rep["edge"]
        out["gated_all"][idx] = rep["gated_all"]
    loss = (cur * g32.to(device=device, dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, [x0] + [P[k] for k in NET_NAMES], allow_unused=True)
    out["xk"] = cur.detach().cpu().numpy()
    out["gx"] = grads[0].cpu().numpy()
    for k, gr in zip(NET_NAMES, grads[1:]):
        out[k] = (torch.zeros_like(P[k]) if gr is None else gr).cpu().numpy()
    return out


def grouped64(field, x, t, t_target, g, dtype=torch.float64, device="cpu"):
    """the defining form: advect64.advect64 per distinct (t, t_target) group, xk / gx scattered back, the net gradients summed over the groups"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    g = np.asarray(g, np.float32).reshape(-1, 3)
    N = x.shape[0]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    out = dict(xk=np.zeros((N, 3), npdt), gx=np.zeros((N, 3), npdt), n_rejected=0, edge=np.zeros(N, bool), gated_all=np.ones(N, bool), n_outside=0)
    for ta, tb, idx in groups_of(as_times(t, N), as_times(t_target, N)):
        y = a64.advect64(field, x[idx], ta, tb, g[idx], dtype=dtype, device=device)
        out["xk"][idx], out["gx"][idx] = y["xk"], y["gx"]
        out["edge"][idx], out["gated_all"][idx] = y["edge"], y["gated_all"]
        out["n_rejected"] += y["n_rejected"]
        out["n_outside"] += y["n_outside"]
        for k in NET_NAMES:
            out[k] = y[k] if k not in out else out[k] + y[k]
    return out


def floors(y32, y64):
    return a64.floors(y32, y64)


# ---------------------------------------------------------------------------------------------------------------- the cases of the goldens
# The plain-fp32 noise floor of the golden cases (xk, gx, worst net tensor), measured on the CPU by tests/golden/make_golden_advect_pt.py, rounded
# up to two digits; tests/test_advect_pt_golden.py measures them again and fails when one exceeds its entry here.
GOLDEN_FLOOR = {
    "A:mixed": (9.4e-8, 1.4e-7, 5.2e-7), "B:mixed": (1.3e-7, 2.0e-7, 4.4e-7),
    "A:distinct": (6.2e-8, 1.4e-7, 9.7e-7), "B:distinct": (1.1e-7, 1.1e-7, 8.9e-7),
}
# (the reference's own fp32 run sits at 6.3e-8 .. 1.3e-7 (xk), 1.1e-7 .. 2.0e-7 (gx) and 2.5e-7 .. 3.8e-7 (worst net tensor) from the float64 run)
T_NONKEY = 19.0 / 60.0


def time_pairs(kind, ts):
    """the five (t, t_target) pairs of tests/golden/make_golden_advect.py: cases_of(kind, ts)"""
    return [(T_NONKEY, T_NONKEY), (T_NONKEY, T_NONKEY + ts / 4), (T_NONKEY, T_NONKEY - 1.3 * ts), (45.0 / 60.0, 45.0 / 60.0 + 0.2),
            (0.0, 1.0 if kind == "A" else 4.5 * ts)]


def mixed_times(kind, ts, N, offset=0):
    """point i takes pair (i + offset) % 5 -> (t, t_target), float32"""
    pairs = np.array(time_pairs(kind, ts), np.float64).astype(np.float32)
    k = (np.arange(N) + offset) % 5
    return pairs[k, 0].copy(), pairs[k, 1].copy()


def distinct_times(tmax, ts, N=97):
    """97 distinct pairs: t uniform in [0, tmax), the target within +- 2.2 ts of it, float32"""
    rng = np.random.default_rng(1257)
    t = rng.random(N) * tmax
    t1 = t + (rng.random(N) * 4.4 - 2.2) * ts
    return t.astype(np.float32), t1.astype(np.float32)


def case_of(kind, name, tmax, ts):
    """x, g, t, t_target of a golden case"""
    N = 257 if name == "mixed" else 97
    x, g = a64.case_inputs(N)
    t, t1 = mixed_times(kind, ts, N) if name == "mixed" else distinct_times(tmax, ts, N)
    return x, g, t, t1


def golden_net(gold_dir, case):
    import os
    kind, name = case.split(":")
    z = np.load(os.path.join(gold_dir, f"advect_pt_net_{kind}.npz"))
    return {k: z[f"{case}:{k}"] for k in NET_NAMES}
