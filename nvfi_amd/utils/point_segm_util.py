"""utils/point_segm_util.py of the reference (test_segm_render.py:123-130 aligns the predicted objects' order with the ground truth's before it
draws them): compress_label and align_insts with the reference's signatures, and the same alignment computed from a confusion matrix, which is
all it depends on - SegmEvaluator sums the kernel's per-frame matrices and relabels on the device through the look-up table."""
import numpy as np

from .metric_segm import linear_assignment


def compress_label(segm):
    """labels -> their ranks among the labels that occur (np.unique's inverse)"""
    return np.unique(segm, return_inverse=True)[1]


def align_lut_from_confusion(counts):
    """counts (G, K) summed over all frames -> lut (K,) int64: predicted class -> index of the ground-truth object (among those that occur) it
    is matched with by the largest total overlap; a class that never occurs maps to 0."""
    counts = np.asarray(counts, np.int64)
    gi, pj = np.nonzero(counts.sum(1))[0], np.nonzero(counts.sum(0))[0]
    n = max(gi.size, pj.size)
    overlap = np.zeros((n, n))
    overlap[:gi.size, :pj.size] = counts[np.ix_(gi, pj)]
    row, col = linear_assignment(overlap, maximize=True)
    lut = np.zeros(counts.shape[1], np.int64)
    for r, c in zip(row, col):
        if c < pj.size:
            lut[pj[c]] = r
    return lut


def align_insts(gt_segm, segm):
    """gt_segm, segm: integer label arrays of one shape (host arrays, labels compressed as the reference's caller does) -> segm renumbered so that
    every predicted object carries the index of the ground-truth object it overlaps most, the assignment being optimal over all objects"""
    gt_segm, segm = np.asarray(gt_segm), np.asarray(segm)
    g, p = compress_label(gt_segm.reshape(-1)), compress_label(segm.reshape(-1))
    ng, npred = int(g.max()) + 1, int(p.max()) + 1
    counts = np.bincount(g * npred + p, minlength=ng * npred).reshape(ng, npred)
    lut = align_lut_from_confusion(counts)
    # (as in the reference, segm is compared with the compressed index itself: its caller passes compressed labels)
    out = np.zeros_like(segm)
    for c in range(npred):
        out[segm == c] = lut[c]
    return out
