#!/usr/bin/env python
"""Differentiable advection with per-point times (field.advect_pt: nvfi_integrate_pos forward, nvfi_advect_pt_steps + nvfi_advect_grad_pt backward;
csrc/advect_pt.hip) at N = 262 144 points on the bench's bat scene (bench.build_scene: 199^3 grid, K = 16), timed on the GPU for three time sets:
  scalar     one scalar pair (1.25 ts -> 1.25 ts + 1.75 ts / 2 ... four RK2 steps, as tools/bench_advect.py): compared with field.advect, which does
             the same work - the difference is the histogram read, the sort and the schedule table
  keyframe   60 frame times, every point to the nearest keyframe of its own frame
  random     60 random pairs, the target within +- 2.2 ts of t
For the last two the comparison figure is the only route without advect_pt: one field.advect call per distinct pair on that pair's points, summed.
  forward             under no_grad: integrate_pos (per-group loop: one integrate_pos per pair)
  forward + backward  value, g_x and the 12 gradients of weight_net
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds; workspace bytes and the chunk list are printed.
    python tools/bench_advect_pt.py [--out profiles/advect_pt_timing.txt] [--max-workspace-bytes B]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_advect import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-workspace-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_advect_pt needs the GPU: there is no CPU fallback"
    import bench
    model = bench.build_scene("cuda")
    f = model.nvfi
    f.eval()
    K, N = int(f.num_keyframes), a.points
    ts = float(f.tmax) / (K - 1)
    torch.manual_seed(0)
    pts = (torch.rand(N, 3, device="cuda") * 2 - 1).requires_grad_(True)
    g = torch.randn(N, 3, device="cuda")
    params = list(f.vel_net.weight_net.parameters())
    rng = np.random.default_rng(7)
    frames = (np.arange(60) / 59.0 * float(f.tmax)).astype(np.float32)
    which = torch.from_numpy(rng.integers(0, 60, N)).cuda()
    t_rand = (rng.random(60) * float(f.tmax)).astype(np.float32)
    sets = {
        "scalar": (np.float32([1.25 * ts]), np.float32([1.25 * ts + 3.5 * ts / 2])),
        "keyframe": (frames, (np.rint(frames / np.float32(ts)) * np.float32(ts)).astype(np.float32)),
        "random": (t_rand, (t_rand + (rng.random(60) * 4.4 - 2.2) * ts).astype(np.float32)),
    }
    lines = [f"differentiable advection with per-point times, N = {N}, bat scene {f.gridSize.tolist()} K = {K}; {torch.cuda.get_device_name(0)}; "
             f"max_workspace_bytes = {a.max_workspace_bytes}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max]"]
    for name, (ta, tb) in sets.items():
        idx = which % len(ta)
        t, t1 = torch.from_numpy(ta).cuda()[idx], torch.from_numpy(tb).cuda()[idx]
        groups = [(float(ta[k]), float(tb[k]), torch.nonzero(idx == k)[:, 0]) for k in range(len(ta))]
        gp = [(u, v, pts.detach()[ix].requires_grad_(True), g[ix]) for u, v, ix in groups]

        def fwd():
            with torch.no_grad():
                return f.advect_pt(pts, t, t1)

        def both():
            y = f.advect_pt(pts, t, t1, max_workspace_bytes=a.max_workspace_bytes)
            return torch.autograd.grad((y * g).sum(), [pts] + params)

        def loop_fwd():
            with torch.no_grad():
                return [f.advect(x, u, v) for u, v, x, _ in gp]

        def loop_both():
            tot = None
            for u, v, x, gg in gp:
                y = f.advect(x, u, v, max_workspace_bytes=a.max_workspace_bytes)
                gr = torch.autograd.grad((y * gg).sum(), [x] + params, allow_unused=True)
                tot = gr[1:] if tot is None else [p if q is None else q if p is None else p + q for p, q in zip(tot, gr[1:])]
            return tot

        for _ in range(2):
            fwd(); both(); loop_fwd(); loop_both()
        torch.cuda.synchronize()
        chunks, ws = list(f.last_advect_pt_chunks), f.last_advect_pt_workspace_bytes
        work = sum(n * s for n, s in chunks)
        tf, tb_ = timed(fwd, a.reps, a.rounds), timed(both, a.reps, a.rounds)
        lf, lb = timed(loop_fwd, a.reps, a.rounds), timed(loop_both, a.reps, a.rounds)
        steps = sorted({s for _, s in chunks}, reverse=True)
        lines.append(f"{name:9s} {len(ta):2d} pair(s), step counts {steps}, {work} point-steps in {len([c for c in chunks if c[1]])} launched chunk(s), workspace {ws} bytes")
        lines.append(f"          advect_pt            forward {tf[0]:9.1f} us [{tf[1]:.1f} .. {tf[2]:.1f}] | forward + backward {tb_[0]:10.1f} us [{tb_[1]:.1f} .. {tb_[2]:.1f}]"
                     f" = {tb_[0] * 1e3 / max(work, 1):.2f} ns / point / step")
        lines.append(f"          advect per pair      forward {lf[0]:9.1f} us [{lf[1]:.1f} .. {lf[2]:.1f}] | forward + backward {lb[0]:10.1f} us [{lb[1]:.1f} .. {lb[2]:.1f}]"
                     f" = {lb[0] / tb_[0]:.2f} x advect_pt")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
