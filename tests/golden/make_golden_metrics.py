#!/usr/bin/env python
"""Golden vectors of the evaluation metrics, generated from the REFERENCE implementation (utils/metrics.py: SSIM; utils/metric_segm.py:
accumulate_eval_results, calculate_AP, calculate_PQ_F1, ClusteringMetrics; utils/point_segm_util.py: align_insts - PyTorch CPU, numpy, scipy):
    python tests/golden/make_golden_metrics.py        (NVFI_REFERENCE: checkout of the reference; default as in make_golden.py)
The reference modules import cv2, imageio and lpips, which nothing here uses: the script puts empty stand-ins into sys.modules.  scipy and
matplotlib (the reference's own dependencies) are needed to RUN this script, not by the product or the tests.

Writes tests/golden/metrics.npz (numbers only).
  ssim:<name>:*   image pairs (C, H, W) and the reference's (ssim, cs) in fp32; `ssim:window2d` / `ssim:window1d` the reference's windows;
                  `ssim:dev` the largest distance of the fp32 reference from the float64 yardstick (tests/metrics64.py) over the pairs, for
                  (ssim, cs) - the test bounds are derived from it.
  segm:<name>:*   mask (B, N, K), segm (B, N), the threshold, and the reference's Pred_IoU, Pred_Matched, Confidence, N_GT_Inst, AP, PQ, F1, Pre,
                  Rec, per-frame IoU and RI of ClusteringMetrics (both specs: these frames are small enough for its N x N form), their means,
                  and align_insts' output; counts (B, G, K): the intersections restated from the full arrays the way eval_segm counts them.
                  `segm:conf_dev`: the largest relative distance of the reference's fp32 confidences from the yardstick's float64 ones.
It ASSERTS the conditions that make AP and the matching well-posed, so that fp32-versus-fp64 rounding of a confidence cannot reorder anything:
confidences of a case pairwise >= 1e-4 apart, no IoU within 1e-6 of 0.5, a unique optimal assignment among the labels that occur (all optimal
assignments share their non-zero entries).  These are conditions on the inputs, checked against the reference alone."""
import importlib.util
import itertools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402
import metrics64 as m64  # noqa: E402

REF = os.environ.get("NVFI_REFERENCE", make_golden.REF)


def load_reference():
    sys.dont_write_bytecode = True
    for name in ("cv2", "imageio", "lpips"):
        sys.modules.setdefault(name, types.ModuleType(name))
    mods = {}
    for name in ("metrics", "metric_segm", "point_segm_util"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "utils", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods


# ---------------------------------------------------------------- inputs
def image_pair(rng, C, H, W, lo, hi, noise):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.stack([0.5 + 0.25 * np.sin(0.21 * (c + 1) * x + 0.4 * c) * np.cos(0.17 * y * (1 + 0.3 * c)) + 0.2 * ((x // 9 + y // 7) % 2) for c in range(C)])
    gt = np.clip(gt + 0.03 * rng.standard_normal(gt.shape), 0, 1)
    pred = np.clip(gt + noise * rng.standard_normal(gt.shape) + 0.02 * np.sin(0.05 * x * y / max(H, W)), 0, 1)
    return (lo + (hi - lo) * pred).astype(np.float32), (lo + (hi - lo) * gt).astype(np.float32)


def label_frame(rng, h, w, objects):
    """background 0 and discs / boxes with labels 1.. (later ones on top); `objects`: (label, cy, cx, radius, box?)"""
    y, x = np.mgrid[0:h, 0:w]
    lab = np.zeros((h, w), np.int64)
    for label, cy, cx, r, box in objects:
        inside = (np.abs(y - cy) <= r) & (np.abs(x - cx) <= r) if box else (y - cy) ** 2 + (x - cx) ** 2 <= r * r
        lab[inside] = label
    return lab


def mask_for(rng, lab, K, perm, shift, sharp, flip=0.03, zero_bg=False, dead=()):
    """softmax mask whose argmax is the ground truth moved by `shift` pixels, renamed through `perm`, with a fraction `flip` of random pixels;
    class k wins with a margin of about sharp[k], so the mean winning value differs per class"""
    h, w = lab.shape
    moved = np.roll(lab, shift, axis=(0, 1))
    want = np.asarray(perm)[moved]
    rnd = rng.random((h, w)) < flip
    live = [k for k in range(K) if k not in dead]
    want[rnd] = rng.choice(live, size=int(rnd.sum()))
    z = 0.3 * rng.standard_normal((h, w, K))
    z[np.arange(h)[:, None], np.arange(w)[None, :], want] += np.asarray(sharp)[want] + 0.4 * rng.random((h, w))
    for k in dead:
        z[..., k] = -30.0
    e = np.exp(z - z.max(-1, keepdims=True))
    m = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    if zero_bg:       # the composited map of a ray that hits nothing: all zeros
        m[(moved == 0) & ~rnd] = 0.0
    return m.reshape(h * w, K)


def segm_cases():
    rng = np.random.default_rng(20240)
    cases = {}
    h, w = 36, 44
    objs = [(1, 9, 10, 6, False), (2, 24, 14, 7, True), (3, 12, 32, 8, False), (4, 28, 34, 5, True)]
    sharp8 = [2.0, 2.6, 3.3, 1.5, 4.0, 2.3, 3.0, 1.8]
    lab = label_frame(rng, h, w, objs)
    cases["basic"] = dict(mask=mask_for(rng, lab, 8, [5, 2, 0, 7, 3], (1, 2), sharp8)[None], segm=lab.reshape(1, -1), thresh=0)
    cases["empty_pred"] = dict(mask=mask_for(rng, lab, 6, [0, 1, 2, 4, 5], (2, -1), sharp8[:6], dead=(3,))[None], segm=lab.reshape(1, -1), thresh=0)
    cases["zero_bg"] = dict(mask=mask_for(rng, lab, 5, [0, 3, 1, 2, 4], (0, 1), sharp8[:5], flip=0.02, zero_bg=True)[None], segm=lab.reshape(1, -1), thresh=0)
    lab_s = label_frame(rng, h, w, objs[:3] + [(4, 30, 36, 1, True)])          # object 4: nine pixels, inside the background's prediction
    cases["ignore"] = dict(mask=mask_for(rng, lab_s, 7, [0, 4, 2, 6, 0], (1, 0), sharp8[:7], flip=0.01)[None], segm=lab_s.reshape(1, -1), thresh=20)
    frames = [label_frame(rng, h, w, objs), label_frame(rng, h, w, [(1, 20, 12, 8, True), (3, 10, 30, 6, False), (5, 27, 33, 6, False)]),
              label_frame(rng, h, w, [(2, 8, 8, 5, False), (4, 18, 22, 9, True), (5, 29, 38, 4, True)])]
    sharp_f = [sharp8, [2.2, 3.1, 1.7, 2.8, 3.6, 1.4, 2.5, 3.9], [3.4, 1.6, 2.9, 2.1, 1.9, 3.7, 2.7, 1.3]]
    shifts = [(1, 1), (0, 3), (4, 2)]         # the third frame's objects are moved far enough that some IoU fall below 0.5
    cases["multi"] = dict(mask=np.stack([mask_for(rng, f, 8, [0, 6, 1, 4, 2, 7], s, sh) for f, s, sh in zip(frames, shifts, sharp_f)]),
                          segm=np.stack([f.reshape(-1) for f in frames]), thresh=0)
    lab2 = label_frame(rng, 30, 33, [(1, 14, 16, 9, False)])
    cases["two"] = dict(mask=mask_for(rng, lab2, 2, [1, 0], (1, 1), [2.0, 3.0])[None], segm=lab2.reshape(1, -1), thresh=0)
    lab8 = label_frame(rng, h, w, objs + [(5, 5, 22, 3, True), (6, 31, 6, 3, False), (7, 19, 40, 3, True)])
    cases["full8"] = dict(mask=mask_for(rng, lab8, 8, [7, 6, 5, 4, 3, 2, 1, 0], (3, 2), sharp8, flip=0.05)[None], segm=lab8.reshape(1, -1), thresh=0)
    return cases


# ---------------------------------------------------------------- well-posedness
def assert_unique_assignment(iou, label):
    """all optimal assignments of the matrix (rows -> distinct columns) share their non-zero entries"""
    iou = np.asarray(iou, np.float64)
    if iou.shape[0] > iou.shape[1]:
        iou = iou.T
    r, c = iou.shape
    best, sets = -1.0, []
    for cols in itertools.permutations(range(c), r):
        v = iou[np.arange(r), cols].sum()
        if v > best + 1e-9:
            best, sets = v, []
        if v >= best - 1e-9:
            sets.append(frozenset((i, j) for i, j in enumerate(cols) if iou[i, j] > 0))
    assert len(set(sets)) == 1, (label, "optimal assignment is not unique", len(set(sets)))


def main():
    R = load_reference()
    out = {}
    # ---- SSIM
    rng = np.random.default_rng(7)
    ssim = R["metrics"].SSIM()
    out["ssim:window1d"] = ssim.gaussian(11, 1.5).numpy()
    out["ssim:window2d"] = ssim.create_window(11, 1)[0, 0].numpy()
    pairs = {"unit48": image_pair(rng, 3, 48, 48, 0.0, 1.0, 0.05), "wide": image_pair(rng, 3, 37, 61, 0.0, 1.0, 0.10),
             "bytes": image_pair(rng, 3, 40, 45, 0.0, 255.0, 0.04), "signed1": image_pair(rng, 1, 64, 50, -1.0, 1.0, 0.08),
             "smooth4": image_pair(rng, 4, 33, 29, 0.0, 1.0, 0.01)}
    dev = np.zeros(2)
    for name, (p, g) in pairs.items():
        s, cs = ssim(torch.from_numpy(p)[None], torch.from_numpy(g)[None], full=True)
        y = m64.ssim64(p, g, out["ssim:window2d"])
        L = m64.derived_range(p)
        d = np.abs(np.array([float(s), float(cs)]) - np.array(y))
        dev = np.maximum(dev, d)
        print(f"[ssim] {name}: {p.shape}, L = {L}; reference fp32 ssim {float(s):.8f} cs {float(cs):.8f}; float64 {y[0]:.10f} {y[1]:.10f}; distance {d[0]:.2e} {d[1]:.2e}")
        out[f"ssim:{name}:pred"], out[f"ssim:{name}:gt"] = p, g
        out[f"ssim:{name}:ref"] = np.array([float(s), float(cs)], np.float64)
        out[f"ssim:{name}:L"] = np.int64(L)
    assert {int(out[f"ssim:{n}:L"]) for n in pairs} == {1, 2, 255}
    out["ssim:dev"] = dev
    out["ssim:names"] = np.array(list(pairs))
    print(f"[ssim] reference fp32 against the float64 yardstick, worst over the pairs: ssim {dev[0]:.2e}, cs {dev[1]:.2e}")
    # ---- segmentation
    ms = R["metric_segm"]
    cases = segm_cases()
    conf_dev = 0.0
    for name, c in cases.items():
        mask, segm, thresh = c["mask"], c["segm"], c["thresh"]
        B, N, K = mask.shape
        G = int(segm.max()) + 1
        assert 2 <= K <= 8 and 2 <= G <= 8
        tm, ts = torch.from_numpy(mask), torch.from_numpy(segm)
        assert np.array_equal(tm.argmax(-1).numpy(), mask.argmax(-1))
        iou, matched, conf, n_gt = ms.accumulate_eval_results(ts, tm, ignore_npoint_thresh=thresh)
        AP = ms.calculate_AP(matched, conf, n_gt)
        PQ, F1, Pre, Rec = ms.calculate_PQ_F1(iou, matched, n_gt)
        cm = ms.ClusteringMetrics()(tm, ts, ignore_npoint_thresh=thresh)
        counts = np.zeros((B, G, K), np.int64)
        for b in range(B):
            pred = mask[b].argmax(1)
            for g in range(G):
                for k in range(K):
                    counts[b, g, k] = np.sum(np.logical_and(segm[b] == g, pred == k))
        # the yardstick's float64 confidences against the reference's, and the well-posedness of the case
        from nvfi_amd.utils import metric_segm as own
        y = [m64.confusion64(mask[b], segm[b], G) for b in range(B)]
        assert all(np.array_equal(y[b][0], counts[b]) for b in range(B))
        _, _, conf64, _ = own.accumulate_from_confusion([yy[0] for yy in y], [yy[1] for yy in y], thresh)
        assert conf64.shape == conf.shape, (name, "a prediction was dropped: the reference's confidence indexing is off there (metric_segm.py docstring)")
        conf_dev = max(conf_dev, float(np.max(np.abs(conf64 - conf) / conf)))
        gaps = np.diff(np.sort(conf))
        assert gaps.min() >= 1e-4, (name, "confidences too close", gaps.min())
        assert np.abs(iou - 0.5).min() > 1e-6, (name, "an IoU sits at the 0.5 threshold")
        for b in range(B):
            gi, pj = np.nonzero(counts[b].sum(1))[0], np.nonzero(counts[b].sum(0))[0]
            sub = counts[b][np.ix_(gi, pj)].astype(np.float64)
            sizes = sub.sum(1)
            if thresh > 0:
                sub = sub[sizes >= thresh]
            assert_unique_assignment(sub / (sub.sum(1)[:, None] + sub.sum(0)[None, :] - sub), f"{name}[{b}]")
        gt_c = R["point_segm_util"].compress_label(segm.reshape(-1))
        pr_c = R["point_segm_util"].compress_label(mask.reshape(-1, K).argmax(-1))
        assert_unique_assignment(np.array([[np.sum((gt_c == i) & (pr_c == j)) for j in range(pr_c.max() + 1)] for i in range(gt_c.max() + 1)]), name + " align")
        aligned = R["point_segm_util"].align_insts(gt_c, pr_c)
        print(f"[segm] {name}: B={B} N={N} K={K} G={G} thresh={thresh}; {conf.shape[0]} predictions, {int(matched.sum())} matched of {n_gt} objects; "
              f"AP {AP:.6f} PQ {PQ:.6f} F1 {F1:.6f} Pre {Pre:.4f} Rec {Rec:.4f} mIoU {np.mean(cm['iou']):.6f} RI {np.mean(cm['ri']):.6f}; "
              f"min confidence gap {gaps.min():.2e}, min |IoU - 0.5| {np.abs(iou - 0.5).min():.2e}")
        pre = f"segm:{name}:"
        out.update({pre + "mask": mask, pre + "segm": segm.astype(np.int32), pre + "thresh": np.int64(thresh), pre + "counts": counts,
                    pre + "Pred_IoU": iou, pre + "Pred_Matched": matched, pre + "Confidence": conf, pre + "N_GT_Inst": np.int64(n_gt),
                    pre + "scores": np.array([AP, PQ, F1, Pre, Rec, np.mean(cm["iou"]), np.mean(cm["ri"])], np.float64),
                    pre + "iou": np.array(cm["iou"], np.float64), pre + "ri": np.array(cm["ri"], np.float64), pre + "aligned": aligned.astype(np.int32)})
    c = cases
    assert (c["empty_pred"]["mask"].argmax(-1) != 3).all() and (c["zero_bg"]["mask"].max(-1) == 0).sum() > 100
    small = np.bincount(c["ignore"]["segm"][0])
    assert 0 < small[4] < c["ignore"]["thresh"] and c["multi"]["mask"].shape[0] == 3
    out["segm:conf_dev"] = np.float64(conf_dev)
    out["segm:names"] = np.array(list(cases))
    print(f"[segm] reference fp32 confidences against the float64 yardstick, worst relative distance: {conf_dev:.2e}")
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
