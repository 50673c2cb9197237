#!/usr/bin/env python
"""One call of the characteristic loss (value + gradients of the twelve planes and basis_mat, csrc/charloss.hip) at N = 262 144 points on the
bench's bat scene (bench.build_scene: 199^3 grid, K = 16), at keyframe k = 1 and k = K - 1, timed on the GPU and split into its two parts:
  warp   field.integrate_pos(points, t_k, 0) alone - the launch path the call uses; 2 k RK2 steps, so it dominates at large k
  loss   the call minus the warp: the two gather / scatter kernels, the clear and the finish
There is no earlier GPU implementation to compare with.  --cpu-reference DIR times the reference's pieces (integrate_pos,
compute_densityfeature, compute_appfeature, autograd backward; eval mode, cloned arguments) on the CPU at --cpu-points points of the same
recipe on a reference-built field, as BASELINE.md does for the other terms; DIR is a checkout of the reference.
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds.  Prints a table; --out writes it to a file.
    python tools/bench_charloss.py [--out profiles/charloss_timing.txt] [--once]   (--once: one warm call per time, for a kernel trace)"""
import argparse
import os
import sys
import time

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


def cpu_reference(ref_dir, n_pts, K=16, tmax=0.75):
    """seconds per call of the reference's pieces on the CPU, per keyframe row (1, K - 1)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    mg.REF = ref_dir
    R = mg.import_reference()
    cfg, nv = mg.build_field(R, "B")          # K = 16, the reference's own constructor; 16..18^3 grid: the gathers do not depend on the grid size
    f = nv.nvfi
    f.eval()
    ts = f.tmax / (f.num_keyframes - 1)
    out = {}
    for row in (1, f.num_keyframes - 1):
        pts = torch.rand(n_pts, 3) * 2 - 1
        tt = torch.full((n_pts, 1), row * ts)
        t0 = time.perf_counter()
        nv.zero_grad(set_to_none=True)
        with torch.no_grad():
            p0 = f.integrate_pos(pts.clone(), tt.clone(), (tt * 0).clone())
        t1 = time.perf_counter()
        qt = torch.cat([pts, f.normalize_time_coord(tt)], -1)
        q0 = torch.cat([p0, f.normalize_time_coord(tt * 0)], -1)
        loss = torch.mean((f.compute_densityfeature(qt) - f.compute_densityfeature(q0)) ** 2) + \
            torch.mean((f.compute_appfeature(qt) - f.compute_appfeature(q0)) ** 2)
        loss.backward()
        t2 = time.perf_counter()
        out[row] = (t1 - t0, t2 - t1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cpu-reference", metavar="DIR")
    ap.add_argument("--cpu-points", type=int, default=262144)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_charloss needs the GPU: there is no CPU fallback"
    import bench
    model = bench.build_scene("cuda")
    f = model.nvfi
    K, N = int(f.num_keyframes), a.points
    ts = float(f.tmax) / (K - 1)
    torch.manual_seed(0)
    pts = torch.rand(N, 3, device="cuda") * 2 - 1
    zeros = torch.zeros(N, device="cuda")
    lines = [f"characteristic loss, value + gradients (fused form), N = {N}, bat scene {f.gridSize.tolist()} K = {K}; {torch.cuda.get_device_name(0)}; "
             f"HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max]"]
    for row in (1, K - 1):
        t = row * ts
        tk = torch.full((N,), f.characteristic_time(t), device="cuda")
        full = lambda: f.characteristic_loss_backward_(pts, t, weight=1.0)       # noqa: E731
        warp = lambda: f.integrate_pos(pts, tk, zeros)                           # noqa: E731
        for _ in range(3):
            full(); warp()
        torch.cuda.synchronize()
        if a.once:
            continue
        tf, tw = timed(full, a.reps, a.rounds), timed(warp, a.reps, a.rounds)
        terms = f.last_char_terms.cpu().numpy()
        lines.append(f"k = {row:2d} ({2 * row:2d} RK2 steps): call {tf[0]:9.1f} us [{tf[1]:.1f} .. {tf[2]:.1f}] | warp alone {tw[0]:9.1f} us [{tw[1]:.1f} .. {tw[2]:.1f}] | "
                     f"loss kernels (difference) {tf[0] - tw[0]:9.1f} us = {(tf[0] - tw[0]) * 1e3 / N:.2f} ns / point | terms {terms[0]:.4e} {terms[1]:.4e}")
    if a.cpu_reference and not a.once:
        ref = cpu_reference(a.cpu_reference, a.cpu_points, K)
        for row, (tw, tl) in ref.items():
            lines.append(f"reference pieces on the CPU ({torch.get_num_threads()} threads), N = {a.cpu_points}, k = {row}: warp {tw:.2f} s | loss + backward {tl:.2f} s")
    if not a.once:
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
