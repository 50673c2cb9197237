#!/usr/bin/env python
"""One call of the distortion loss on ray weights, value + gradient, at (R, S) = (2 048, 128) and (2 048, 686) (training batches of the
shipped configs) and (32 768, 128) (an evaluation chunk), timed on the GPU three ways on the same weights:
  hip     utils.distortion_loss(w, delta) + .backward(): nvfi_ray_distortion value-only forward (two launches), one gradient launch backward
  raw     one nvfi_ray_distortion call with value and gradient (what render_mse_backward_(..., distortion_weight=) adds to a fused step)
  torch   the same loss written in fp32 torch ops on the same device (cumsum form, torch_form() below) + .backward()
Inputs: weights of a seeded density profile (alpha * T of a thin background and two bumps per ray).  The torch form also gives the value the
other two are checked against (1e-5 relative) before anything is timed.
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds.  Prints a table; --out writes it to a file.
    python tools/bench_rayregs.py [--out profiles/rayregs_timing.txt]"""
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


def torch_form(w, delta):
    """the same loss in torch ops: A = exclusive prefix sum of the inclusive prefix sum of w, D_r = delta [2 sum w A + 1/3 sum w^2]"""
    winc = w.cumsum(1)
    A = winc.cumsum(1) - winc
    return (delta * (2.0 * (w * A).sum(1) + (w * w).sum(1) / 3.0)).mean()


def make_weights(R, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    j = torch.arange(S, device="cuda")[None, :].float()
    c = torch.rand(R, 2, device="cuda", generator=g) * S
    alpha = 0.5 / S * (0.5 + torch.rand(R, S, device="cuda", generator=g))
    for k in range(2):
        alpha = alpha + 0.3 * torch.exp(-0.5 * ((j - c[:, k:k + 1]) / (S / 64.0 + 0.5)) ** 2)
    alpha = alpha.clamp(0.0, 1.0)
    T = torch.cumprod(torch.cat([torch.ones(R, 1, device="cuda"), 1.0 - alpha[:, :-1]], 1), 1)
    return (alpha * T).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 128, 2048, 686, 32768, 128], help="R S pairs")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rayregs needs the GPU: there is no CPU fallback"
    from nvfi_amd.utils.ray_regs import distortion_loss, distortion_loss_raw, distortion_workspace
    lines = [f"distortion loss on ray weights, value + gradient; {torch.cuda.get_device_name(0)}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max], us per call"]
    for R, S in zip(a.sizes[0::2], a.sizes[1::2]):
        delta = 1.0 / S
        w = make_weights(R, S, R + S).requires_grad_(True)
        wd = w.detach()
        out = (torch.empty((), device="cuda"), torch.empty(R, S, device="cuda"))
        ws = distortion_workspace(R, "cuda")

        def hip():
            w.grad = None
            distortion_loss(w, delta).backward()

        def raw():
            distortion_loss_raw(wd, delta, out=out, workspace=ws)

        def ref():
            w.grad = None
            torch_form(w, delta).backward()

        for _ in range(3):
            hip(); raw(); ref()
        torch.cuda.synchronize()
        v_hip, v_ref = float(distortion_loss(wd, delta)), float(torch_form(wd, delta))
        assert abs(v_hip - v_ref) <= 1e-5 * abs(v_ref), (R, S, v_hip, v_ref)
        th, tr, tt = timed(hip, a.reps, a.rounds), timed(raw, a.reps, a.rounds), timed(ref, a.reps, a.rounds)
        lines.append(f"R = {R:6d} S = {S:4d}: hip {th[0]:8.1f} [{th[1]:.1f} .. {th[2]:.1f}] | raw call {tr[0]:8.1f} [{tr[1]:.1f} .. {tr[2]:.1f}] | "
                     f"torch ops {tt[0]:8.1f} [{tt[1]:.1f} .. {tt[2]:.1f}] | torch / hip {tt[0] / th[0]:.2f} | torch / raw {tt[0] / tr[0]:.2f} | "
                     f"loss {v_hip:.6f} (torch {v_ref:.6f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
