#!/usr/bin/env python
"""Differentiable field lookups (field.lookup_density / lookup_appfeature: nvfi_density_at + nvfi_density_grad, nvfi_appfeat_at + nvfi_appfeat_grad;
csrc/lookup.hip) at N = 262 144 uniform points on the bench's bat scene (bench.build_scene: 199^3 grid, K = 16), timed on the GPU, once with
fractional time rows (t' uniform in [-1, 1]) and once on a keyframe row:
  forward             under no_grad
  forward + backward  value, then the gradients of sum(feat * g) to the points, the six planes of the family and (appearance) basis_mat.weight
next to the same lookups written with F.grid_sample + autograd on the device, on the field's own parameters (the reference's
compute_densityfeature / compute_appfeature, models/tensorf_keyframe.py:233-310).
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds.  Prints a table; --out writes it to a file.
    python tools/bench_lookup.py [--out profiles/lookup_timing.txt] [--points 262144 4096 ...]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAT_SPACE, MAT_TIME = [(0, 1), (0, 2), (1, 2)], [(2, 3), (1, 3), (0, 3)]


def timed(fn, reps, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def torch_lookup(f, q, family):
    """the reference's lookup in torch ops on the field's own (channels_last) planes"""
    space, time = (f.density_plane_space, f.density_plane_time) if family == "density" else (f.app_plane_space, f.app_plane_time)
    out = None
    for i in range(3):
        a = F.grid_sample(space[i], q[:, list(MAT_SPACE[i])].view(1, -1, 1, 2), align_corners=True).view(space[i].shape[1], q.shape[0])
        b = F.grid_sample(time[i], q[:, list(MAT_TIME[i])].view(1, -1, 1, 2), align_corners=True).view(time[i].shape[1], q.shape[0])
        out = a * b if out is None else out * (a * b)
    return out.sum(0).unsqueeze(-1) if family == "density" else f.basis_mat(out.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--points", type=int, nargs="+", default=[262144])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lookup needs the GPU: there is no CPU fallback"
    import bench
    model = bench.build_scene("cuda")
    f = model.nvfi
    f.eval()
    K = int(f.num_keyframes)
    params = {"density": list(f.density_plane_space) + list(f.density_plane_time),
              "app": list(f.app_plane_space) + list(f.app_plane_time) + [f.basis_mat.weight]}
    lines = [f"differentiable field lookups, bat scene {f.gridSize.tolist()} K = {K}; {torch.cuda.get_device_name(0)}; HIP events, median of {a.rounds} rounds x "
             f"{a.reps} calls [min .. max], us; hip = csrc/lookup.hip, torch = F.grid_sample + autograd on the same parameters"]
    for N in a.points:
        torch.manual_seed(0)
        base = torch.rand(N, 4, device="cuda") * 2 - 1
        for rows in ("fractional", "keyframe"):
            q0 = base.clone()
            if rows == "keyframe":
                q0[:, 3] = 2.0 * (K // 3) / (K - 1) - 1.0
            q = q0.requires_grad_(True)
            for family in ("density", "app"):
                hip = f.lookup_density if family == "density" else f.lookup_appfeature
                ref = lambda x, fam=family: torch_lookup(f, x, fam)                                   # noqa: E731
                with torch.no_grad():
                    width = hip(q).shape[1]
                g = torch.randn(N, width, device="cuda")
                cell = []
                for fn in (hip, ref):
                    def fwd(fn=fn):
                        with torch.no_grad():
                            return fn(q)

                    def both(fn=fn):
                        return torch.autograd.grad((fn(q) * g).sum(), [q] + params[family])

                    for _ in range(3):
                        fwd(); both()
                    torch.cuda.synchronize()
                    cell.append((timed(fwd, a.reps, a.rounds), timed(both, a.reps, a.rounds)))
                (hf, hb), (tf, tb) = cell
                lines.append(f"N = {N:7d} {rows:10s} {family:8s}: forward hip {hf[0]:8.1f} [{hf[1]:.1f} .. {hf[2]:.1f}] torch {tf[0]:8.1f} [{tf[1]:.1f} .. {tf[2]:.1f}] | "
                             f"forward + backward hip {hb[0]:8.1f} [{hb[1]:.1f} .. {hb[2]:.1f}] torch {tb[0]:8.1f} [{tb[1]:.1f} .. {tb[2]:.1f}] | "
                             f"torch / hip {tf[0] / hf[0]:.2f}x, {tb[0] / hb[0]:.2f}x")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
