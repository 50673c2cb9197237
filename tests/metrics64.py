"""float64 numpy yardstick of the two kernel stages of csrc/metrics.hip (no torch, no GPU): what tests/test_metrics_golden.py pins to the reference's
outputs (tests/golden/metrics.npz) and tests/test_gpu_metrics.py holds the kernels to.

ssim64: the reference's formula (utils/metrics.py:32-99) with its fp32 2-D window promoted to float64 - the dense 121-tap sum, no separable
    short-cut - everything else in float64.
confusion64: argmax (numpy: lowest index on ties), counts[g][k], conf_sum[k] and the predicted labels by plain loops and np.add.at."""
import numpy as np


def derived_range(pred):
    """the reference's rule (metrics.py:57-66)"""
    return (255 if pred.max() > 128 else 1) - (-1 if pred.min() < -0.5 else 0)


def ssim64(pred, gt, window2d, L=None):
    """pred, gt (C, H, W) -> (mean SSIM, mean cs) of one image in float64"""
    p, g, w = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(window2d, np.float64)
    if L is None:
        L = derived_range(np.asarray(pred))
    n = w.shape[0]
    C, H, W = p.shape
    oh, ow = H - n + 1, W - n + 1

    def conv(x):
        out = np.zeros((C, oh, ow))
        for i in range(n):
            for j in range(n):
                out += w[i, j] * x[:, i:i + oh, j:j + ow]
        return out

    mu1, mu2 = conv(p), conv(g)
    s1, s2, s12 = conv(p * p) - mu1 * mu1, conv(g * g) - mu2 * mu2, conv(p * g) - mu1 * mu2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    return float((((2 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2)).mean()), float((v1 / v2).mean())


def confusion64(mask, segm, G, loops=True):
    """mask (N, K) float32, segm (N,) integers -> counts (G, K) int64, conf_sum (K,) float64, pred (N,) int64, number of labels outside [0, G);
    loops=False takes np.argmax (the same rule) for frames too large for a Python loop"""
    mask, segm = np.asarray(mask), np.asarray(segm).astype(np.int64)
    N, K = mask.shape
    pred = np.argmax(mask, axis=1).astype(np.int64)
    for n in range(N if loops else 0):
        best = 0
        for k in range(1, K):
            if mask[n, k] > mask[n, best]:
                best = k
        pred[n] = best
    ok = (segm >= 0) & (segm < G)
    counts = np.zeros((G, K), np.int64)
    np.add.at(counts, (segm[ok], pred[ok]), 1)
    conf = np.zeros(K, np.float64)
    np.add.at(conf, pred[ok], mask[np.arange(N), pred][ok].astype(np.float64))
    return counts, conf, pred, int((~ok).sum())
