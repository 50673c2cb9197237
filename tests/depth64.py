"""float64 yardstick of the depth loss (csrc/depthloss.hip: nvfi_depth_loss; reference utils/evaluation_utils.py:8-17 compute_depth_loss):
numpy only.  The median is torch.median's LOWER median (sorted element (n_c - 1) // 2) and its gradient is spread equally over all entries
equal to it, which is what torch autograd does for the full-tensor median:

    e_j = [p_j == med] / c        a_j = 2 (u_j - v_j) / n_c       A = sum a_j      B = sum a_j (p_j - med)      sg_j = sign(p_j - med)
    dL/dp_j = a_j / (s + eps) - e_j A / (s + eps) - B / (s + eps)^2 (sg_j - e_j sum(sg)) / n_c

gt_index gathers the target (gt[gt_index]); skip_holes counts entry j only if its target is finite and > 0.  Entries that do not count get a
gradient of exactly 0; with nothing counted the loss is 0."""
import numpy as np

EPS = 1e-6


def counted_mask(gt, skip_holes):
    gt = np.asarray(gt, np.float64).ravel()
    if not skip_holes:
        return np.ones(gt.shape, bool)
    with np.errstate(invalid="ignore"):
        return np.isfinite(gt) & (gt > 0)


def lower_median(x):
    return np.sort(x)[(x.size - 1) // 2]


def depth64(pred, gt, gt_index=None, skip_holes=False):
    """-> dict(loss, grad (n,), n_counted, med_pred, med_gt); inputs of any float type, flattened, evaluated in float64"""
    p_all = np.asarray(pred, np.float64).ravel()
    g_all = np.asarray(gt, np.float64).ravel()
    if gt_index is not None:
        g_all = g_all[np.asarray(gt_index, np.int64).ravel()]
    assert p_all.shape == g_all.shape, (p_all.shape, g_all.shape)
    m = counted_mask(g_all, skip_holes)
    grad = np.zeros(p_all.shape, np.float64)
    nc = int(m.sum())
    if nc == 0:
        return dict(loss=0.0, grad=grad, n_counted=0, med_pred=np.nan, med_gt=np.nan, grad_floor=0.0)
    p, g = p_all[m], g_all[m]
    with np.errstate(invalid="ignore", divide="ignore"):
        if np.isnan(p).any() or np.isnan(g).any():
            grad[m] = np.nan
            return dict(loss=np.nan, grad=grad, n_counted=nc, med_pred=np.nan, med_gt=np.nan, grad_floor=0.0)
        med_p, med_g = lower_median(p), lower_median(g)
        dp = p - med_p
        inv_p = 1.0 / (np.mean(np.abs(dp)) + EPS)
        inv_g = 1.0 / (np.mean(np.abs(g - med_g)) + EPS)
        d = dp * inv_p - (g - med_g) * inv_g
        a = 2.0 * d / nc
        tie = p == med_p
        e = tie / float(tie.sum())
        sg = np.sign(dp)
        A, B = a.sum(), (a * dp).sum()
        grad[m] = a * inv_p - e * A * inv_p - B * inv_p * inv_p * (sg - e * sg.sum()) / nc
        # the size of the terms the gradient is a sum of, BEFORE u - v cancels: 2 max(|u|, |v|) / (n_c (s + eps))
        floor = 2.0 * max(np.abs(dp * inv_p).max(), np.abs((g - med_g) * inv_g).max()) * inv_p / nc
    return dict(loss=float(np.mean(d * d)), grad=grad, n_counted=nc, med_pred=float(med_p), med_gt=float(med_g), grad_floor=float(floor))


ILL_CONDITIONED = 2.0 ** -10


def grad_scale(y):
    """what a gradient error is measured against: max|grad| of the yardstick - unless the gradient is a cancellation of more than 10 bits of
    its own terms (max|grad| < 2^-10 grad_floor), then grad_floor, the size of those terms.  fp32 arithmetic rounds each term to 2^-24 of ITS
    size, so below that line an error relative to max|grad| measures rounding noise against rounding noise: with n = 2 the normalised map is
    (0, 2) whatever the two depths are, the exact gradient is ~0 (only the 1e-6 in the denominator moves it), and the reference's fp32
    gradient there is 1e-2 of max|grad| = 3e-8 of its terms."""
    gmax = float(np.max(np.abs(y["grad"]))) if y["grad"].size else 0.0
    return gmax if gmax >= ILL_CONDITIONED * y["grad_floor"] else y["grad_floor"]


def errors(loss, grad, y):
    """(absolute error of the loss, error of the gradient relative to grad_scale(y): max|grad| of the yardstick on every well-conditioned case)"""
    e_loss = abs(float(loss) - y["loss"])
    e_abs = float(np.max(np.abs(np.asarray(grad, np.float64).ravel() - y["grad"]))) if y["grad"].size else 0.0
    sc = grad_scale(y)
    return e_loss, (e_abs / sc if sc > 0 else e_abs)


def error_vs_gmax(grad, y):
    """the gradient error relative to max|grad| with no floor (documentation: make_golden_depth.py stores its maximum as ref32_err:grad_raw)"""
    gmax = float(np.max(np.abs(y["grad"]))) if y["grad"].size else 0.0
    e_abs = float(np.max(np.abs(np.asarray(grad, np.float64).ravel() - y["grad"]))) if y["grad"].size else 0.0
    return e_abs / gmax if gmax > 0 else e_abs


def named_case(name, n, seed, far=8.0):
    """seeded fp32 (pred, gt) of the named cases of tests/golden/make_golden_depth.py and tests/test_gpu_depthloss.py"""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(1.0, far, n).astype(np.float32)
    gt = rng.uniform(1.0, far, n).astype(np.float32)
    if name == "distinct":
        pass
    elif name == "plateau":          # 60 % of pred equal to far: the median lies in the ties
        k = max(1, int(round(0.6 * n)))
        pred[rng.permutation(n)[:k]] = np.float32(far)
    elif name == "allequal":
        pred[:] = np.float32(3.25)
    elif name == "signed":           # negative values, -0.0 and +0.0 among the entries (about a fifth each: the median is a zero)
        pred = rng.uniform(-4.0, 4.0, n).astype(np.float32)
        gt = rng.uniform(-4.0, 4.0, n).astype(np.float32)
        perm = rng.permutation(n)
        k = max(1, n // 5)
        pred[perm[:k]] = np.float32(-0.0)
        pred[perm[k:2 * k]] = np.float32(0.0)
        gt[perm[-k:]] = np.float32(-0.0)
    else:
        raise ValueError(name)
    return pred, gt
