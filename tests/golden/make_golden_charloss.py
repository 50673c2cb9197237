#!/usr/bin/env python
"""Golden vectors of the characteristic loss (nvfi_char_loss), generated from the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_charloss.py        (reference checkout as in make_golden.py)
The reference's own characteristic_loss (models/tensorf_keyframe.py:552-573) aliases its arguments: integrate_pos writes into `t` (and, in
training mode, into the points), so the method compares keyframe ~0 with keyframe 0.  The goldens hold the semantics of its
FORMULA instead, assembled from the reference's pieces with cloned arguments in eval mode: its snap lines, integrate_pos,
normalize_time_coord, compute_densityfeature, compute_appfeature, autograd.  Fields: the two golden fields of make_golden.py, A (K = 4,
VelocityAABB) and B (K = 16, VelocityAABBSur), with the LAST layer of the shared velocity net (weight and bias) multiplied by `<kind>:vel_scale`
so that points travel far enough to leave the box (A).  Writes tests/golden/charloss.npz (numbers only), per case <kind>:<case>:
  points, t, t_k, row, points0, loss_d, loss_a, gradnorm:<tensor> (L2), ref32_err:<quantity>, shipped_train / shipped_eval, and for the case
  `kmax` grad:<tensor> (every gradient in full).
  ref32_err     rel_err (char64.rel_err: max-norm error over max-norm) of the reference's fp32 result against char64 (float64) on the same
                points / points0, for both loss terms and each of the 13 gradient tensors: the reference's distance from exact arithmetic
  <kind>:ref32_err:<quantity>  the maximum of ref32_err over the field's cases
  shipped_*     what the reference's own characteristic_loss(N, t) returns under torch.manual_seed(SEED) in train / eval mode: documentation only
Cases (ts = tmax / (K - 1)): k1 t = ts | kmax t = tmax (row K-1; A: 1 %..50 % of points0 outside the box) | up t = 1.6 ts (snaps upward to row 2)
| zero t = 0 and neg t = -1 (the ts branch, row 1) | snap0 t = 0.3 ts (snaps to row 0: exact zeros) | out (B only) t = ts with points drawn
from [-1.08, 1.08]^3: with the surround box no step can leave the box, so the zero-padded taps of B are reached by points that start outside
(they sit outside the gate and do not move: points0 = points there).
ASSERTS: the snap restated in char64.snap_time gives the reference's t_k; kmax (A) / out (B) have 1 %..50 % of points0 outside [-1,1]^3; the
N = 1000 point sets hold a point exactly on a box face; every loss term of a non-zero case is above 1e-8."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import char64 as c64  # noqa: E402

SEED = 1234
VEL_SCALE = {"A": 6.0, "B": 6.0}


def scale_vel(f, s):
    last = f.vel_net.weight_net[-1][0]
    with torch.no_grad():
        last.weight.mul_(s)
        last.bias.mul_(s)


def snap_ref(f, N, t):
    """the reference's lines 554-561, restated"""
    if t > 0:
        tt = torch.ones(N, 1) * t
        ts = f.tmax / (f.num_keyframes - 1) if f.num_keyframes > 1 else 1
        return torch.round((tt / ts).clamp(0.0, f.num_keyframes - 1)) * ts
    return torch.ones(N, 1) * f.tmax / (f.num_keyframes - 1)


def reference_terms(nv, points, tt):
    """both terms, points0 and every gradient from the reference's pieces (fp32, eval mode, cloned arguments)"""
    f = nv.nvfi
    f.eval()
    nv.zero_grad(set_to_none=True)
    t0 = tt * 0.
    with torch.no_grad():
        points0 = f.integrate_pos(points.clone(), tt.clone(), t0.clone())
    qt = torch.cat([points, f.normalize_time_coord(tt)], -1)
    q0 = torch.cat([points0, f.normalize_time_coord(t0)], -1)
    loss_d = torch.mean((f.compute_densityfeature(qt) - f.compute_densityfeature(q0)) ** 2)
    loss_a = torch.mean((f.compute_appfeature(qt) - f.compute_appfeature(q0)) ** 2)
    (loss_d + loss_a).backward()
    named = dict(nv.named_parameters())
    grads = {}
    for n in c64.NAMES:
        p = named["nvfi." + n]
        grads[n] = np.zeros(tuple(p.shape), np.float32) if p.grad is None else mg.npf(p.grad)
    for k, p in named.items():
        assert "vel" not in k or p.grad is None, k         # nothing reaches the velocity nets
    return dict(loss_d=float(loss_d), loss_a=float(loss_a), grads=grads), points0


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    fx = {}
    for kind, nv in (("A", nvA), ("B", nvB)):
        f = nv.nvfi
        scale_vel(f, VEL_SCALE[kind])
        fx[f"{kind}:vel_scale"] = np.float64(VEL_SCALE[kind])
        K, tmax = f.num_keyframes, f.tmax
        ts = tmax / (K - 1)
        params = c64.params_from_sd({k: mg.npf(v) for k, v in nv.state_dict().items()})
        gen = torch.Generator().manual_seed(SEED + (0 if kind == "A" else 1))
        cases = [("k1", ts, 1000, 1.0), ("kmax", tmax, 1000, 1.0), ("up", 1.6 * ts, 65, 1.0), ("zero", 0.0, 63, 1.0), ("neg", -1.0, 1, 1.0),
                 ("snap0", 0.3 * ts, 63, 1.0)]
        if kind == "B":
            cases.append(("out", ts, 1000, 1.08))
        for name, t, N, half in cases:
            points = (torch.rand(N, 3, generator=gen) * 2 - 1) * half
            if N >= 1000:
                points[0] = torch.tensor([1.0, 0.3, -0.2])
                points[1, 1] = -1.0
                assert bool((points.abs() == 1).any())
            tt = snap_ref(f, N, t)
            t_k, row = c64.snap_time(K, tmax, t)
            assert float(tt[0, 0]) == t_k and bool((tt == tt[0, 0]).all()), (kind, name, float(tt[0, 0]), t_k)
            ref, points0 = reference_terms(nv, points, tt)
            y64 = c64.char64(params, K, points.numpy(), points0.numpy(), row)
            err = c64.errors(ref, y64)
            key = f"{kind}:{name}"
            fx[key + ":points"], fx[key + ":points0"] = mg.npf(points), mg.npf(points0)
            fx[key + ":t"], fx[key + ":t_k"], fx[key + ":row"] = np.float64(t), np.float64(t_k), np.int64(row)
            fx[key + ":loss_d"], fx[key + ":loss_a"] = np.float32(ref["loss_d"]), np.float32(ref["loss_a"])
            for q, e in err.items():
                fx[f"{key}:ref32_err:{q}"] = np.float64(e)
            for n in c64.NAMES:
                fx[f"{key}:gradnorm:{n}"] = np.float64(np.linalg.norm(ref["grads"][n].astype(np.float64)))
                if name == "kmax":
                    fx[f"{key}:grad:{n}"] = ref["grads"][n]
            # the reference's own method, as shipped (documentation): same seed, train and eval mode
            for mode in ("train", "eval"):
                getattr(f, mode)()
                torch.manual_seed(SEED)
                with torch.no_grad():
                    fx[f"{key}:shipped_{mode}"] = np.float32(float(f.characteristic_loss(N, t)))
            f.eval()
            frac = c64.outside_fraction(points0.numpy())
            moved = float((points0 - points).norm(dim=-1).max())
            print(f"{key}: t={t:.4f} t_k={t_k:.6f} row={row} N={N} loss_d={ref['loss_d']:.6e} loss_a={ref['loss_a']:.6e} "
                  f"yardstick=({y64['loss_d']:.6e}, {y64['loss_a']:.6e}) outside={frac:.3f} max|x0-x|={moved:.3f} "
                  f"shipped train/eval={float(fx[key + ':shipped_train']):.3e}/{float(fx[key + ':shipped_eval']):.3e}")
            print("    ref32_err: " + " ".join(f"{q.replace('_plane_', '.').replace('grad:', '')}={e:.1e}" for q, e in err.items()))
            if row == 0:
                assert ref["loss_d"] == 0.0 and ref["loss_a"] == 0.0 and all(not g.any() for g in ref["grads"].values())
            else:
                assert ref["loss_d"] > 1e-8 and ref["loss_a"] > 1e-8, (key, ref["loss_d"], ref["loss_a"])
            if (kind, name) in (("A", "kmax"), ("B", "out")):
                assert 0.01 <= frac <= 0.5, (key, frac)
        # per field and quantity: the largest error the reference shows over the field's cases (the bound of the GPU test, whose sizes and
        # times are not all golden cases)
        for q in list(c64.TERMS) + ["grad:" + n for n in c64.NAMES]:
            fx[f"{kind}:ref32_err:{q}"] = np.float64(max(float(fx[f"{kind}:{name}:ref32_err:{q}"]) for name, *_ in cases))
    path = os.path.join(HERE, "charloss.npz")
    np.savez_compressed(path, **fx)
    print("wrote charloss.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
