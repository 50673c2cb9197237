#!/usr/bin/env python
"""One call of the depth loss, value + gradient, at n = 2 048 (a training batch), 16 384 (the largest size the kernel keeps in LDS) and
640 000 (an 800 x 800 evaluation frame), timed on the GPU two ways on the same inputs:
  hip     utils.compute_depth_loss(pred, gt) + .backward(): one nvfi_depth_loss launch (csrc/depthloss.hip) and one scaling launch
  raw     the nvfi_depth_loss launch alone (what render_mse_backward_(..., target_depth=) adds to a fused step)
  torch   the same loss written in torch ops on the same device (normalised() below, applied to both maps) + .backward()
Inputs: depths in [1, 8] with 60 % of pred on a plateau at 8 (rays that hit nothing), gt seeded uniform.  The torch form also gives the
value the other two are checked against (1e-5 relative) before anything is timed.
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds.  Prints a table; --out writes it to a file.
    python tools/bench_depthloss.py [--out profiles/depthloss_timing.txt]"""
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


def normalised(x):
    """a map shifted to its (lower) median and divided by its mean absolute deviation"""
    centred = x - x.median()
    return centred / (centred.abs().mean() + 1e-6)


def torch_form(pred, gt):
    """the same loss in torch ops: mean squared difference of the two normalised maps"""
    return (normalised(pred) - normalised(gt)).square().mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 16384, 640000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depthloss needs the GPU: there is no CPU fallback"
    from nvfi_amd.utils.evaluation_utils import compute_depth_loss, depth_loss_raw
    lines = [f"depth loss, value + gradient; {torch.cuda.get_device_name(0)}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max], us per call"]
    for n in a.sizes:
        g = torch.Generator(device="cuda").manual_seed(n)
        pred = torch.rand(n, device="cuda", generator=g) * 7 + 1
        pred[torch.rand(n, device="cuda", generator=g) < 0.6] = 8.0
        pred.requires_grad_(True)
        gt = torch.rand(n, device="cuda", generator=g) * 7 + 1
        out = (torch.empty((), device="cuda"), torch.empty(n, device="cuda"), torch.empty((), dtype=torch.int64, device="cuda"))
        pd = pred.detach()

        def hip():
            pred.grad = None
            compute_depth_loss(pred, gt).backward()

        def raw():
            depth_loss_raw(pd, gt, None, False, 1.0, out=out)

        def ref():
            pred.grad = None
            torch_form(pred, gt).backward()

        for _ in range(3):
            hip(); raw(); ref()
        torch.cuda.synchronize()
        v_hip, v_ref = float(compute_depth_loss(pd, gt)), float(torch_form(pd, gt))
        assert abs(v_hip - v_ref) <= 1e-5 * abs(v_ref), (n, v_hip, v_ref)
        th, tr, tt = timed(hip, a.reps, a.rounds), timed(raw, a.reps, a.rounds), timed(ref, a.reps, a.rounds)
        lines.append(f"n = {n:7d}: hip {th[0]:8.1f} [{th[1]:.1f} .. {th[2]:.1f}] | raw launch {tr[0]:8.1f} [{tr[1]:.1f} .. {tr[2]:.1f}] | "
                     f"torch ops {tt[0]:8.1f} [{tt[1]:.1f} .. {tt[2]:.1f}] | torch / hip {tt[0] / th[0]:.2f} | loss {v_hip:.6f} (torch {v_ref:.6f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
