#!/usr/bin/env python
"""Differentiable advection (field.advect: nvfi_integrate_pos forward, nvfi_advect_grad backward; csrc/advect.hip) at N = 262 144 points on the
bench's bat scene (bench.build_scene: 199^3 grid, K = 16), one and four RK2 steps, timed on the GPU:
  forward             field.advect under no_grad: the launch path of integrate_pos
  forward + backward  value, g_x and the 12 gradients of weight_net: the forward again, then per chunk the stash-writing warp on the uniform
                      schedule, the unfused adjoint and the six weight-gradient jobs + slab reduce
Counting only, forward + backward is 2 x steps net evaluations forward, the same again for the recompute, and the adjoint plus six weight-gradient
contractions: what a render's warp + unfused adjoint do on an equal list.  There is no earlier GPU implementation to compare with.
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds; the workspace bytes and the chunk count are printed.
    python tools/bench_advect.py [--out profiles/advect_timing.txt] [--max-workspace-bytes B]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-workspace-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_advect needs the GPU: there is no CPU fallback"
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
    t = 1.25 * ts
    lines = [f"differentiable advection, N = {N}, bat scene {f.gridSize.tolist()} K = {K}; {torch.cuda.get_device_name(0)}; max_workspace_bytes = "
             f"{a.max_workspace_bytes}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max]"]
    for steps in (1, 4):
        t1 = t + (steps - 0.5) * ts / 2          # steps - 1 full steps of ts / 2 and half a step

        def fwd():
            with torch.no_grad():
                return f.advect(pts, t, t1)

        def both():
            y = f.advect(pts, t, t1, max_workspace_bytes=a.max_workspace_bytes)
            return torch.autograd.grad((y * g).sum(), [pts] + params)

        for _ in range(3):
            fwd(); both()
        torch.cuda.synchronize()
        tf, tb = timed(fwd, a.reps, a.rounds), timed(both, a.reps, a.rounds)
        lines.append(f"{steps} RK2 step(s): forward {tf[0]:9.1f} us [{tf[1]:.1f} .. {tf[2]:.1f}] | forward + backward {tb[0]:9.1f} us [{tb[1]:.1f} .. {tb[2]:.1f}] = "
                     f"{tb[0] * 1e3 / N / steps:.2f} ns / point / step | workspace {f.last_advect_workspace_bytes} bytes, {f.last_advect_chunks} chunk(s)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
