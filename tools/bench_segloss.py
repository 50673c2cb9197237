#!/usr/bin/env python
"""Forward + backward of the three segmentation losses (train_segm.py:182-202), timed two ways on the GPU:
  hip    nvfi_amd.utils.seg_loss.segm_losses - one neighbour search, one fused forward + backward (csrc/segloss.hip);
  torch  the same losses written in torch ops - what a user had before the kernels existed: a dense N x N distance matrix + topk for the
         neighbours, torch.linalg.svd for the fit, autograd for the gradient.  Kept here, not in the package.
Sizes: the shipped N (the occupied points of the 64^3 lattice of the bench's bat-box scene, ~1e4; here a shell of a jittered 64^3 lattice of that
size) and 32 768 points.  One process, warm-up, HIP events around `reps` steps, the median of `rounds` rounds, the two paths alternating.
Launch counts come from torch.profiler's kernel list of one step.  Prints a table; --out writes it to a file.
    python tools/bench_segloss.py [--out profiles/segloss_timing.txt] [--once hip]   (--once: one warm step of one path, for a kernel trace)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nvfi_amd.utils import seg_loss as sl  # noqa: E402


def make_inputs(n_target, K=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = 64
    edges = torch.linspace(-1.0, 1.0, n + 1)
    ax = edges[:-1, None] + (edges[1:, None] - edges[:-1, None]) * torch.rand(n, 3, generator=g)
    x, y, z = torch.meshgrid(ax[:, 0], ax[:, 1], ax[:, 2], indexing="ij")
    p = torch.stack([x, y, z], -1).reshape(-1, 3)
    r = p.norm(dim=1)
    order = torch.argsort((r - 0.6).abs())[:n_target]          # the n_target lattice points closest to the sphere r = 0.6: a shell
    pc = p[torch.sort(order).values].contiguous()
    W = torch.randn(3, K, generator=g) * 3.0
    logits = torch.tanh(pc @ torch.randn(3, 32, generator=g) * 2.0) @ torch.randn(32, K, generator=g) * 0.7 + pc @ W
    flow = 0.03 * torch.stack([-pc[:, 1], pc[:, 0], 0.3 * pc[:, 2]], 1) + 1e-3 * torch.randn(pc.shape, generator=g)
    return pc.cuda()[None], flow.cuda()[None], logits.cuda()


def torch_losses(pc, mask, flow, k, radius, smooth_w, entropy_w):
    """the reference's formulation in torch ops on the GPU (B = 1)"""
    p, m, f = pc[0], mask[0], flow[0]
    N, K = m.shape
    p2 = p + f
    with torch.no_grad():
        w = m.detach().t()                                      # (K, N)
        sw = w.sum(1, keepdim=True)
        mu1, mu2 = (w @ p) / sw, (w @ p2) / sw
        c1, c2 = p[None] - mu1[:, None], p2[None] - mu2[:, None]
        S = c1.transpose(1, 2) @ (w[:, :, None] * c2)
        valid = ~torch.isnan(S).flatten(1).any(1)
        U, _, Vh = torch.linalg.svd(torch.where(valid[:, None, None], S, torch.eye(3, device=S.device).expand_as(S)))
        V = Vh.transpose(1, 2)
        det = torch.det(V @ U.transpose(1, 2))
        D = torch.diag_embed(torch.stack([torch.ones_like(det), torch.ones_like(det), det], 1))
        R = V @ D @ U.transpose(1, 2)
        t = mu2 - (R @ mu1[:, :, None])[:, :, 0]
        eye = torch.eye(3, device=S.device).expand_as(R)
        R = torch.where(valid[:, None, None], R, eye)
        t = torch.where(valid[:, None], t, torch.zeros_like(t))
        T = torch.einsum("kij,nj->kni", R, p) + t[:, None]
        d2 = (p * p).sum(1)[:, None] + (p * p).sum(1)[None] - 2.0 * (p @ p.t())      # the dense N x N matrix
        dist, idx = torch.topk(d2, k, dim=1, largest=False)
        idx = torch.where(dist > radius, idx[:, :1].expand_as(idx), idx)
    q = (m.t()[:, :, None] * T).sum(0)
    l_dyn = (q - p2).norm(dim=-1).mean()
    l_sm = (m[:, None, :] - m[idx]).norm(p=1, dim=-1).mean()
    l_en = -(m * torch.log(m.clamp(1e-5))).sum(-1).mean()
    return l_dyn + smooth_w * l_sm + entropy_w * l_en, torch.stack([l_dyn, l_sm, l_en]).detach()


def step(path, pc, flow, logits, k, radius, sw, ew):
    logits.grad = None
    mask = torch.softmax(logits, -1)[None]
    if path == "hip":
        loss, parts = sl.segm_losses(pc, mask, flow, k, radius, sw, ew)
        parts = parts[0]
    else:
        loss, parts = torch_losses(pc, mask, flow, k, radius, sw, ew)
    loss.backward()
    return loss.detach(), parts


def count_kernels(path, args):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(path, *args)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(ev), sum(1 for e in ev if e.name.startswith("k_seg") or "k_zero_words" in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--once", choices=["hip", "torch"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segloss needs the GPU: there is no CPU fallback"
    k, radius, sw, ew = 4, 0.01, 0.1, 0.0
    lines = [f"segmentation losses, forward + backward incl. softmax of the logits and the neighbour search (k={k}, radius={radius}, K=8); "
             f"{torch.cuda.get_device_name(0)}; HIP events, median of {a.rounds} rounds x {a.reps} steps, paths alternating"]
    for n_target in (9000, 32768):
        pc, flow, logits = make_inputs(n_target)
        logits.requires_grad_(True)
        args = (pc, flow, logits, k, radius, sw, ew)
        if a.once:
            for _ in range(3):
                step(a.once, *args)
            torch.cuda.synchronize()
            continue
        res = {}
        for path in ("hip", "torch"):
            for _ in range(5):
                res[path] = step(path, *args)
            torch.cuda.synchronize()
        dl = (res["hip"][1] - res["torch"][1]).abs() / res["torch"][1].abs().clamp_min(1e-30)
        times = {"hip": [], "torch": []}
        for _ in range(a.rounds):
            for path in ("hip", "torch"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    step(path, *args)
                e1.record()
                torch.cuda.synchronize()
                times[path].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        med = {p: float(np.median(v)) for p, v in times.items()}
        spread = {p: (float(np.min(v)), float(np.max(v))) for p, v in times.items()}
        nk = {p: count_kernels(p, args) for p in ("hip", "torch")}
        lines.append(f"N = {pc.shape[1]:6d}: hip {med['hip']:8.1f} us [{spread['hip'][0]:.1f} .. {spread['hip'][1]:.1f}], {nk['hip'][0]} launches ({nk['hip'][1]} of segloss.hip)"
                     f" | torch {med['torch']:8.1f} us [{spread['torch'][0]:.1f} .. {spread['torch'][1]:.1f}], {nk['torch'][0]} launches"
                     f" | torch / hip = {med['torch'] / med['hip']:.2f} | losses rel. diff (dynamic, smooth, entropy) {[f'{float(x):.1e}' for x in dl]}")
    if not a.once:
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
