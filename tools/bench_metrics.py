#!/usr/bin/env python
"""The two evaluation metrics per 800 x 800 frame (mask map K = 8, image C = 3), each timed three ways:
  hip    this path: nvfi_amd.utils.metric_segm.segm_confusion / nvfi_amd.utils.metrics.ssim_frames (csrc/metrics.hip), results left on the device;
  torch  the same quantities in torch ops on the device - what a user had before the kernels existed: argmax + bincount(gt * K + argmax) +
         an index-sum of the winning values; five F.conv2d with the 11 x 11 window on the permuted frame.  Kept here, not in the package;
  host   the reference's procedure: copy the frame to the host, then numpy (n_gt x n_pred full-array passes, per-prediction means) and
         torch-CPU conv2d, as utils/metric_segm.py: eval_segm and utils/metrics.py: SSIM do it.  Restated here from their descriptions.
One process; every path warmed up at the timed shape; hip and torch alternate, HIP events around `reps` calls, the median of `rounds` rounds;
the host path is timed with a host clock around work that starts with the device-to-host copy (`host_reps` calls).  Prints ONE JSON line.
    python tools/bench_metrics.py [--out profiles/metrics_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nvfi_amd.utils import metric_segm as ms  # noqa: E402
from nvfi_amd.utils import metrics as mt  # noqa: E402

H = W = 800
K = G = 8


def make_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    segm = (((y // 160) * 2 + (x // 400)) % G).to(torch.int32)
    z = torch.randn(H, W, K, generator=g)
    z.scatter_add_(2, ((segm.long() + (torch.rand(H, W, generator=g) < 0.1)) % K)[..., None], torch.full((H, W, 1), 3.0))
    mask = torch.softmax(z, -1)
    mask[:40] = 0.0
    gt = torch.rand(H, W, 3, generator=g)
    gt = 0.5 * gt + 0.5 * gt.roll(1, 1)
    pred = (gt + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    return mask.cuda(), segm.cuda(), pred.cuda(), gt.cuda()


# ---- segmentation confusion
def segm_hip(mask, segm):
    return ms.segm_confusion(mask.reshape(1, -1, K), segm.reshape(1, -1), G)[:2]


def segm_torch(mask, segm):
    m = mask.reshape(-1, K)
    best, arg = m.max(dim=1)
    counts = torch.bincount(segm.reshape(-1).long() * K + arg, minlength=G * K).reshape(G, K)
    conf = torch.zeros(K, dtype=torch.float64, device=m.device).index_add_(0, arg, best.double())
    return counts, conf


def segm_host(mask, segm):
    m, s = mask.reshape(-1, K).cpu().numpy(), segm.reshape(-1).cpu().numpy()
    pred = np.argmax(m, axis=1)
    _, s, gs = np.unique(s, return_inverse=True, return_counts=True)
    ids, pred, ps = np.unique(pred, return_inverse=True, return_counts=True)
    m = m[:, ids]
    inter = np.zeros((gs.shape[0], ps.shape[0]))
    for i in range(gs.shape[0]):
        for j in range(ps.shape[0]):
            inter[i, j] = np.sum(np.logical_and(s == i, pred == j))
    conf = np.array([np.mean(m[pred == j, j]) for j in range(ps.shape[0])])
    return inter, conf


# ---- SSIM
_WINDOW = {}


def _window(dev, C=3):
    if dev not in _WINDOW:
        _WINDOW[dev] = mt.SSIM().create_window(11, C).to(dev)
    return _WINDOW[dev]


def _ssim_conv(p, g, L=1.0):
    w = _window(p.device, p.shape[1])
    C = p.shape[1]
    mu1, mu2 = F.conv2d(p, w, groups=C), F.conv2d(g, w, groups=C)
    s1 = F.conv2d(p * p, w, groups=C) - mu1 * mu1
    s2 = F.conv2d(g * g, w, groups=C) - mu2 * mu2
    s12 = F.conv2d(p * g, w, groups=C) - mu1 * mu2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    return (((2 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2)).mean()


def ssim_hip(pred, gt):
    return mt.ssim_frames(pred, gt)


def ssim_torch(pred, gt):
    return _ssim_conv(pred.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None])


def ssim_host(pred, gt):
    return _ssim_conv(pred.cpu().permute(2, 0, 1)[None], gt.cpu().permute(2, 0, 1)[None]).item()


def time_device(fns, args, reps, rounds):
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(*args)
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {n: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))} for n, v in times.items()}


def time_host(fn, args, reps):
    torch.cuda.synchronize()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(*args)
        v.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs the GPU: there is no CPU fallback"
    mask, segm, pred, gt = make_inputs()
    res = {"device": torch.cuda.get_device_name(0), "frame": [H, W], "K": K, "G": G, "reps": a.reps, "rounds": a.rounds,
           "host_threads": torch.get_num_threads()}
    for _ in range(10):         # warm-up at the timed shapes: code objects, the allocator, the conv algorithm
        hs, ts = segm_hip(mask, segm), segm_torch(mask, segm)
        hq, tq = ssim_hip(pred, gt), ssim_torch(pred, gt)
    torch.cuda.synchronize()
    # the three paths compute the same thing
    assert torch.equal(hs[0][0], ts[0]) and torch.allclose(hs[1][0], ts[1], rtol=1e-12, atol=0)
    hi, hc = segm_host(mask, segm)
    assert np.array_equal(hi, hs[0][0].cpu().numpy()) and np.allclose(hc, (hs[1][0] / hs[0][0].sum(0)).cpu().numpy(), rtol=1e-5)
    res["ssim_value"] = {"hip": float(hq[0]), "torch": float(tq), "host": ssim_host(pred, gt)}
    assert abs(res["ssim_value"]["hip"] - res["ssim_value"]["torch"]) < 1e-5 and abs(res["ssim_value"]["hip"] - res["ssim_value"]["host"]) < 1e-5
    res["segm"] = time_device({"hip": segm_hip, "torch": segm_torch}, (mask, segm), a.reps, a.rounds)
    res["segm"]["host"] = time_host(segm_host, (mask, segm), a.host_reps)
    res["ssim"] = time_device({"hip": ssim_hip, "torch": ssim_torch}, (pred, gt), a.reps, a.rounds)
    res["ssim"]["host"] = time_host(ssim_host, (pred, gt), a.host_reps)
    for k in ("segm", "ssim"):
        res[k]["torch_over_hip"] = res[k]["torch"]["median_us"] / res[k]["hip"]["median_us"]
        res[k]["host_over_hip"] = res[k]["host"]["median_us"] / res[k]["hip"]["median_us"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
