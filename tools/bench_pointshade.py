#!/usr/bin/env python
"""Differentiable point shading (field.shade / field.lookup_rgb: nvfi_render_mlp + nvfi_render_mlp_grad, csrc/point_shade.hip) at N = 262 144,
16 384 and 1 024 uniform points on the bench's bat scene (bench.build_scene: 199^3 grid, K = 16), timed on the GPU:
  forward             under no_grad
  forward + backward  value, then the gradients of sum(rgb * g): shade - to the features, the points, the view directions and the six MLP tensors;
                      lookup_rgb - to the points (x, y, z, t'), the view directions, the six appearance planes, basis_mat.weight and the MLP
next to the only alternative there was: the same MLP in torch ops (positional encodings, F.linear on the field's own renderModule.mlp parameters,
relu, sigmoid) under autograd - for shade on the same features, for lookup_rgb on field.lookup_appfeature's output.
Counted floor of forward + backward: 2 (110 128 + 128^2 + 128 3) 3 FLOP per point (forward, dgrad, wgrad).
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds.  Prints a table; --out writes it to a file.
    python tools/bench_pointshade.py [--out profiles/pointshade_timing.txt] [--points 262144 16384 1024]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOP_PER_POINT = 2 * (110 * 128 + 128 * 128 + 128 * 3) * 3


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


def _pe(x, n=6):
    f = (x[..., None] * (2.0 ** torch.arange(n, dtype=x.dtype, device=x.device))).reshape(x.shape[0], -1)
    return torch.cat([torch.sin(f), torch.cos(f)], -1)


def torch_shade(f, pts, view, feat):
    """MLPRender_PE.forward (tensorf_base.py:88-98) in torch ops on the field's own parameters"""
    mlp = f.renderModule.mlp
    h = torch.cat([feat, view, pts, _pe(pts), _pe(view)], -1)
    h = F.relu(F.linear(h, mlp[0].weight, mlp[0].bias))
    h = F.relu(F.linear(h, mlp[2].weight, mlp[2].bias))
    return torch.sigmoid(F.linear(h, mlp[4].weight, mlp[4].bias))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--points", type=int, nargs="+", default=[262144, 16384, 1024])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pointshade needs the GPU: there is no CPU fallback"
    import bench
    model = bench.build_scene("cuda")
    f = model.nvfi
    f.eval()
    mlp = [p for i in (0, 2, 4) for p in (f.renderModule.mlp[i].weight, f.renderModule.mlp[i].bias)]
    app = list(f.app_plane_space) + list(f.app_plane_time) + [f.basis_mat.weight]
    lines = [f"differentiable point shading, bat scene {f.gridSize.tolist()} K = {int(f.num_keyframes)}; {torch.cuda.get_device_name(0)}; HIP events, median of "
             f"{a.rounds} rounds x {a.reps} calls [min .. max], us; hip = csrc/point_shade.hip, torch = the MLP in torch ops + autograd on the same parameters; "
             f"counted floor {FLOP_PER_POINT} FLOP per point (forward + dgrad + wgrad)"]
    for N in a.points:
        torch.manual_seed(0)
        q = (torch.rand(N, 4, device="cuda") * 2 - 1).requires_grad_(True)
        view = F.normalize(torch.randn(N, 3, device="cuda"), dim=1).requires_grad_(True)
        feat = f.compute_appfeature(q).requires_grad_(True)
        pts = q.detach()[:, :3].contiguous().requires_grad_(True)
        g = torch.randn(N, 3, device="cuda")
        cases = {
            "shade": ((lambda: f.shade(pts, view, feat)), (lambda: torch_shade(f, pts, view, feat)), [feat, pts, view] + mlp),
            "lookup_rgb": ((lambda: f.lookup_rgb(q, view)), (lambda: torch_shade(f, q[:, :3], view, f.lookup_appfeature(q))), [q, view] + app + mlp),
        }
        for name, (hip, ref, wrt) in cases.items():
            cell = []
            for fn in (hip, ref):
                def fwd(fn=fn):
                    with torch.no_grad():
                        return fn()

                def both(fn=fn):
                    return torch.autograd.grad((fn() * g).sum(), wrt)

                for _ in range(3):
                    fwd(); both()
                torch.cuda.synchronize()
                cell.append((timed(fwd, a.reps, a.rounds), timed(both, a.reps, a.rounds)))
            (hf, hb), (tf, tb) = cell
            lines.append(f"N = {N:7d} {name:10s}: forward hip {hf[0]:8.1f} [{hf[1]:.1f} .. {hf[2]:.1f}] torch {tf[0]:8.1f} [{tf[1]:.1f} .. {tf[2]:.1f}] | "
                         f"forward + backward hip {hb[0]:8.1f} [{hb[1]:.1f} .. {hb[2]:.1f}] torch {tb[0]:8.1f} [{tb[1]:.1f} .. {tb[2]:.1f}] | "
                         f"torch / hip {tf[0] / hf[0]:.2f}x, {tb[0] / hb[0]:.2f}x | hip forward + backward {N * FLOP_PER_POINT / hb[0] * 1e-6:.2f} TFLOP/s of the counted floor")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
