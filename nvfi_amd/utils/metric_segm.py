"""Segmentation metrics of the reference's test_segm_render.py (utils/metric_segm.py: AP@50, PQ@50, F1, Precision, Recall, mIoU, Rand Index)
with its names and signatures, in two stages.

Stage 1 is the kernel nvfi_segm_confusion (csrc/metrics.hip): per frame, from the mask map (N, K) and the ground-truth labels (N,) on the GPU,
    counts[G][K]   pixels with label g whose argmax_k mask is k (ties: lowest index, numpy's rule; an all-zero pixel predicts 0),
    conf_sum[K]    sum of mask[n, argmax] over the pixels predicted k,
and, on request, the predicted label per pixel.  It queues on the current stream and does not wait for the device.  There is no CPU path.
Stage 2 (`*_from_confusion`) is host numpy on those few hundred bytes: every quantity the reference computes from the full arrays is a function
of the two matrices.  It needs neither scipy nor matplotlib: `linear_assignment` is a small O(n^3) solver.

What stage 2 keeps from the reference, on purpose: labels are compacted to those present (np.unique) for AP / PQ; the confidence of a prediction
is the mean of its winning mask values; ClusteringMetrics works in float32 where the reference does (IoU matrix, its mean, the final division
of the Rand Index), so the golden numbers are reproduced to the last bit; its rows are ALL labels below max + 1, present or not.
The Rand Index comes from the confusion matrix: with n_ij the counts, a_i the row and b_j the column sums, the agreeing ordered pairs number
N^2 - sum a_i^2 - sum b_j^2 + 2 sum n_ij^2, exact in integers - the reference's N x N comparison cannot hold a frame (test_segm_render.py:132).
Differences: labels must lie in [0, 32) (G <= 32; K <= 32) - a label outside is reported (NvfiError) when the results are read, a deferred
check; `calculate_AP(plot=True)` raises; with ignore_npoint_thresh > 0 the confidence of a kept prediction is that prediction's own mean (the
reference indexes the pixels of the j-th prediction BEFORE dropping the invalid ones, which mixes two predictions whenever one was dropped)."""

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._lib import stream_ptr as _stream_ptr

MAX_LABELS = 32


# ---------------------------------------------------------------- stage 1: frames -> confusion (GPU)
def segm_confusion(mask, segm, n_gt=None, want_pred=False):
    """mask (B, N, K) float, segm (B, N) integer-valued labels in [0, n_gt), both on the GPU -> device tensors
    counts (B, G, K) int64, conf_sum (B, K) float64, bad (B,) int32 [number of labels outside [0, G)], pred (B, N) int32 or None.
    G = n_gt (default 32, the most the kernel takes).  Nothing is synchronised: check `bad` when the results are read (`confusion_to_host`)."""
    if not (mask.is_cuda and segm.is_cuda):
        raise _lib.NvfiError("the segmentation metrics' confusion stage runs on the GPU only (no CPU fallback exists)")
    if mask.dim() != 3 or segm.dim() != 2 or tuple(mask.shape[:2]) != tuple(segm.shape):
        raise ValueError(f"mask must be (B, N, K) and segm (B, N), got {tuple(mask.shape)} and {tuple(segm.shape)}")
    B, N, K = mask.shape
    G = MAX_LABELS if n_gt is None else int(n_gt)
    if not 1 <= K <= MAX_LABELS or not 1 <= G <= MAX_LABELS:
        raise NotImplementedError(f"1..{MAX_LABELS} predicted classes and ground-truth labels are supported")
    if N == 0 or B == 0:
        raise ValueError("no pixels")
    mask = mask.detach().contiguous().float()
    segm = segm.detach().contiguous().to(torch.int32)
    dev = mask.device
    counts = torch.empty(B, G, K, dtype=torch.int64, device=dev)
    conf = torch.empty(B, K, dtype=torch.float64, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    pred = torch.empty(B, N, dtype=torch.int32, device=dev) if want_pred else None
    lib = _lib.lib()
    nbytes = _lib.bytes_of(lib.nvfi_metrics_workspace_bytes, 1, B, K, 0, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.nvfi_segm_confusion(B, N, K, G, _lib.ptr(mask), _lib.ptr(segm), _lib.ptr(counts), _lib.ptr(conf), _lib.ptr(pred),
                                           _lib.ptr(bad), _lib.ptr(ws), ws.numel(), _stream_ptr()))
    return counts, conf, bad, pred


def confusion_to_host(counts, conf_sum, bad):
    """the one transfer: numpy (counts, conf_sum); raises NvfiError if the kernel met a label outside [0, G)"""
    nbad = bad.cpu().numpy()
    if nbad.any():
        raise _lib.NvfiError(f"nvfi_segm_confusion: {int(nbad.sum())} ground-truth labels outside [0, {counts.shape[-2]}) "
                             f"(frames {np.nonzero(nbad)[0].tolist()}); such pixels were not counted")
    return counts.cpu().numpy(), conf_sum.cpu().numpy()


# ---------------------------------------------------------------- stage 2: confusion -> metrics (host numpy)
def linear_assignment(value, maximize=True):
    """Optimal assignment on a (rows x cols) matrix, every row (or, with more rows than columns, every column) matched once: returns
    (row_ind, col_ind), rows ascending.  Shortest augmenting paths with potentials, O(n^3); meant for n <= 32."""
    value = np.asarray(value, np.float64)
    if value.ndim != 2:
        raise ValueError("a matrix is expected")
    if value.shape[0] > value.shape[1]:
        c, r = linear_assignment(value.T, maximize)
        o = np.argsort(r, kind="stable")
        return r[o], c[o]
    cost = -value if maximize else value
    n, m = cost.shape
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    owner = np.zeros(m + 1, np.int64)          # owner[j]: 1-based row that holds column j (0: free); column 0 is the virtual start
    for i in range(1, n + 1):
        owner[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        way = np.zeros(m + 1, np.int64)
        used = np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = owner[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[owner[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if owner[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            owner[j0] = owner[j1]
            j0 = j1
    col = np.zeros(n, np.int64)
    for j in range(1, m + 1):
        if owner[j]:
            col[owner[j] - 1] = j - 1
    return np.arange(n), col


def eval_segm_from_confusion(counts, conf_sum, ignore_npoint_thresh=0):
    """one frame: counts (G, K), conf_sum (K,) -> pred_iou, pred_matched, confidence (one entry per kept prediction), n_gt_inst - what the
    reference's eval_segm returns for the frame the matrices were counted on"""
    counts = np.asarray(counts, np.int64)
    conf_sum = np.asarray(conf_sum, np.float64)
    gi, pj = np.nonzero(counts.sum(1))[0], np.nonzero(counts.sum(0))[0]        # the labels that occur, ascending: np.unique's compaction
    inter = counts[np.ix_(gi, pj)].astype(np.float64)
    gt_sizes, n_pred_px = inter.sum(1), inter.sum(0)
    small = np.nonzero(gt_sizes < ignore_npoint_thresh)[0]
    in_small = inter[small].sum(0)
    pred_sizes = n_pred_px - in_small                       # a prediction's area inside ignored objects does not count ...
    keep = (pred_sizes > 0) & ~(in_small / n_pred_px > 0.5)  # ... and one that lies mostly there is not a false positive
    inter = np.delete(inter, small, axis=0)[:, keep]
    gt_sizes, pred_sizes = np.delete(gt_sizes, small), pred_sizes[keep]
    confidence = conf_sum[pj][keep] / n_pred_px[keep]
    iou = inter / (gt_sizes[:, None] + pred_sizes[None, :] - inter)
    pred_iou = iou.max(axis=0)
    return pred_iou, (pred_iou >= 0.5).astype(float), confidence, gt_sizes.shape[0]


def accumulate_from_confusion(counts, conf_sum, ignore_npoint_thresh=0):
    """frames (B, G, K), (B, K) -> Pred_IoU, Pred_Matched, Confidence (concatenated over the frames), N_GT_Inst (summed)"""
    res = [eval_segm_from_confusion(c, s, ignore_npoint_thresh) for c, s in zip(counts, conf_sum)]
    return (np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res]),
            int(np.sum([r[3] for r in res])))


def rand_index_counts(counts):
    """(agreeing ordered pairs, all ordered pairs) of the two labellings a confusion matrix was counted on, as exact Python integers:
    pairs together in both + pairs apart in both = N^2 - sum a_i^2 - sum b_j^2 + 2 sum n_ij^2"""
    c = [[int(x) for x in row] for row in np.asarray(counts)]
    n = sum(map(sum, c))
    a2 = sum(sum(row) ** 2 for row in c)
    b2 = sum(sum(col) ** 2 for col in zip(*c))
    return n * n - a2 - b2 + 2 * sum(x * x for row in c for x in row), n * n


def clustering_from_confusion(counts, spec=None, ignore_npoint_thresh=0):
    """one frame: counts (G, K) -> {"iou": mIoU, "ri": Rand Index} as ClusteringMetrics.forward computes them (float32 where it does)"""
    spec = [ClusteringMetrics.IOU, ClusteringMetrics.RI] if spec is None else spec
    counts = np.asarray(counts, np.int64)
    G, K = counts.shape
    present = np.nonzero(counts.sum(1))[0]
    n_gt = int(present[-1]) + 1 if present.size else 1       # the reference's max label + 1: absent labels below it keep their (zero) rows
    k = max(K, n_gt)
    M = np.zeros((k, k), np.int64)
    M[:n_gt, :K] = counts[:n_gt]
    rows = np.ones(n_gt, bool)
    if ignore_npoint_thresh > 0:                             # points of too small objects leave both labellings
        nonsmall = M.sum(1) >= ignore_npoint_thresh
        M[~nonsmall] = 0
        rows = nonsmall[:n_gt]
    out = {}
    if ClusteringMetrics.IOU in spec:
        m32 = M.astype(np.float32)
        union = m32.sum(1, dtype=np.float32)[:, None] + m32.sum(0, dtype=np.float32)[None, :] - m32
        iou = (m32 / (union + np.float32(1e-8)))[:n_gt][rows]
        r, c = linear_assignment(iou, maximize=True)
        out["iou"] = np.mean(iou[r, c])
    if ClusteringMetrics.RI in spec:
        agree, pairs = rand_index_counts(M)
        out["ri"] = float(np.float32(agree) / np.float32(pairs))
    return out


def calculate_AP(Pred_Matched, Confidence, N_GT_Inst, plot=False, eps=1e-10):
    """AP by the MS-COCO rule: predictions by descending confidence (stable), monotone precision envelope, mean over 101 recall thresholds"""
    if plot:
        raise NotImplementedError("plotting is not provided (matplotlib is not a dependency)")
    matched = np.asarray(Pred_Matched, np.float64)[np.argsort(-np.asarray(Confidence), kind="mergesort")]
    tp, fp = np.cumsum(matched), np.cumsum(1 - matched)
    precision = tp / np.maximum(tp + fp, eps)
    recall = tp / N_GT_Inst
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    thresholds = np.linspace(0, 1, 101, endpoint=True)
    at = np.searchsorted(recall, thresholds, side="left")
    queried = np.zeros(thresholds.shape[0])
    hit = at < envelope.shape[0]
    queried[hit] = envelope[at[hit]]
    return np.mean(queried.tolist())


def calculate_PQ_F1(Pred_IoU, Pred_Matched, N_GT_Inst, eps=1e-10):
    Pred_IoU, Pred_Matched = np.asarray(Pred_IoU), np.asarray(Pred_Matched)
    tp = Pred_Matched.sum()
    fp, fn = Pred_Matched.shape[0] - tp, N_GT_Inst - tp
    PQ = Pred_IoU[Pred_Matched > 0].sum() / max(tp + 0.5 * fp + 0.5 * fn, eps)
    Pre, Rec = tp / max(tp + fp, eps), tp / max(tp + fn, eps)
    return PQ, (2 * Pre * Rec) / max(Pre + Rec, eps), Pre, Rec


def summary_from_confusion(counts, conf_sum, ignore_npoint_thresh=0):
    """frames (B, G, K), (B, K) -> the numbers test_segm_render.py prints (and the Rand Index it had to leave out)"""
    iou, matched, conf, n_gt = accumulate_from_confusion(counts, conf_sum, ignore_npoint_thresh)
    PQ, F1, Pre, Rec = calculate_PQ_F1(iou, matched, n_gt)
    per = [clustering_from_confusion(c, None, ignore_npoint_thresh) for c in counts]
    return {"AP": calculate_AP(matched, conf, n_gt), "PQ": PQ, "F1": F1, "Pre": Pre, "Rec": Rec,
            "mIoU": np.mean([[p["iou"]] for p in per]), "RI": np.mean([p["ri"] for p in per]),
            "Pred_IoU": iou, "Pred_Matched": matched, "Confidence": conf, "N_GT_Inst": n_gt}


# ---------------------------------------------------------------- the reference's surface (GPU tensors in, both stages)
def _frames(segm, mask):
    B = mask.shape[0]
    return mask.reshape(B, -1, mask.shape[-1]), segm.reshape(B, -1)


def eval_segm(segm, mask, ignore_npoint_thresh=0):
    """segm (N,), mask (N, K) on the GPU -> pred_iou, pred_matched, confidence, n_gt_inst"""
    counts, conf = confusion_to_host(*segm_confusion(mask[None], segm[None])[:3])
    return eval_segm_from_confusion(counts[0], conf[0], ignore_npoint_thresh)


def accumulate_eval_results(segm, mask, ignore_npoint_thresh=0):
    """segm (B, N), mask (B, N, K) on the GPU -> Pred_IoU, Pred_Matched, Confidence, N_GT_Inst"""
    m, s = _frames(segm, mask)
    counts, conf = confusion_to_host(*segm_confusion(m, s)[:3])
    return accumulate_from_confusion(counts, conf, ignore_npoint_thresh)


class ClusteringMetrics(nn.Module):
    IOU = 1     # mean IoU over an optimal assignment on the IoU matrix
    RI = 2      # Rand Index

    def __init__(self, spec=None):
        super().__init__()
        self.spec = [self.IOU, self.RI] if spec is None else spec

    def forward(self, mask, segm, ignore_npoint_thresh=0):
        """mask (B, ..., K), segm (B, ...) with labels from 0, on the GPU -> {"iou": [per frame], "ri": [per frame]}"""
        m, s = _frames(segm, mask)
        counts, _ = confusion_to_host(*segm_confusion(m, s)[:3])
        per = [clustering_from_confusion(c, self.spec, ignore_npoint_thresh) for c in counts]
        out = {}
        if self.IOU in self.spec:
            out["iou"] = [p["iou"] for p in per]
        if self.RI in self.spec:
            out["ri"] = [p["ri"] for p in per]
        return out


class SegmEvaluator:
    """The evaluation loop of test_segm_render.py:115-180 without leaving the device between frames:
        ev = SegmEvaluator(n_object);  per frame: ev.update(segm_map (H, W, K), gt_segm (H, W));  ev.summary()
    `update` queues one kernel call on the current stream and returns; `summary` brings the matrices of all frames to the host once."""

    def __init__(self, n_object, n_gt=None, keep_labels=False):
        self.n_object, self.n_gt, self.keep_labels = int(n_object), n_gt, keep_labels
        self.frames = []

    def update(self, segm_map, gt_segm):
        if segm_map.shape[-1] != self.n_object or tuple(segm_map.shape[:-1]) != tuple(gt_segm.shape):
            raise ValueError(f"expected a (..., {self.n_object}) mask map and labels of its leading shape, got {tuple(segm_map.shape)}, {tuple(gt_segm.shape)}")
        counts, conf, bad, pred = segm_confusion(segm_map.reshape(1, -1, self.n_object), gt_segm.reshape(1, -1), self.n_gt, self.keep_labels)
        self.frames.append((counts, conf, bad, pred.reshape(gt_segm.shape) if pred is not None else None))

    def confusion(self):
        """(counts (F, G, K), conf_sum (F, K)) of the frames so far, on the host"""
        if not self.frames:
            raise ValueError("no frame has been added")
        return confusion_to_host(torch.cat([f[0] for f in self.frames]), torch.cat([f[1] for f in self.frames]), torch.cat([f[2] for f in self.frames]))

    def summary(self, ignore_npoint_thresh=0, aligned=False):
        """{"AP", "PQ", "F1", "Pre", "Rec", "mIoU", "RI", ...}; with aligned=True (needs keep_labels) also "aligned": the predicted label maps
        (int64 device tensors) renumbered to the ground truth's objects by point_segm_util.align_insts' rule over all frames"""
        counts, conf = self.confusion()
        out = summary_from_confusion(counts, conf, ignore_npoint_thresh)
        if aligned:
            if not self.keep_labels:
                raise ValueError("aligned label maps need SegmEvaluator(..., keep_labels=True)")
            from .point_segm_util import align_lut_from_confusion
            lut = torch.from_numpy(align_lut_from_confusion(counts.sum(0))).to(self.frames[0][3].device)
            out["aligned"] = [lut[f[3].long()] for f in self.frames]
        return out
