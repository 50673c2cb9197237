"""Float64 yardstick of the segmentation objective (the reference's utils/seg_loss.py as train_segm.py:182-202 calls it): a numpy restatement
of dynamic_loss (with fit_motion_svd_batch), smooth_loss and entropy_loss with their gradients w.r.t. the mask, and a brute-force neighbour
search with the ordering the HIP kernels promise.  tests/test_segloss64_golden.py pins it to the reference's own fp32 outputs
(tests/golden/segloss.npz); tests/test_gpu_segloss.py holds the device to it.

Conventions shared with the device and the reference:
  * pc2 = pc + flow is formed in fp32 (the reference does; it is an input of the fit, not part of what is compared);
  * squared distances are formed in fp32 as (dx*dx + dy*dy) + dz*dz and ordered by (distance, index); a slot whose SQUARED distance exceeds
    `radius` (an fp32 comparison) or that does not exist (k > N) holds slot 0's index;
  * the rigid fit is detached: the gradient of the dynamic loss goes through the mask weights only;
  * an object whose 3x3 moment matrix has a NaN keeps R = I, t = 0.
`dtype=np.float32` evaluates the same statements in float32: its distance from the float64 evaluation is the rounding a correct fp32
implementation may show, which is what the GPU tests derive their bounds from."""
import numpy as np


def knn_brute(pc, k, radius, extra=1, chunk=512):
    """-> idx (N,k) int64 with the radius rule applied, raw (N,k+extra) candidate indices (-1: none), d2 (N,k+extra) fp32 (inf: none)"""
    pc = np.asarray(pc, np.float32)
    N = pc.shape[0]
    kk = k + extra
    raw = np.full((N, kk), -1, np.int64)
    d2 = np.full((N, kk), np.inf, np.float32)
    have = min(kk, N)
    for i0 in range(0, N, chunk):
        d = pc[i0:i0 + chunk, None, :] - pc[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.argsort(dd, axis=1, kind="stable")[:, :have]         # stable: equal distances keep the lower index first
        raw[i0:i0 + chunk, :have] = order
        d2[i0:i0 + chunk, :have] = np.take_along_axis(dd, order, 1)
    idx = raw[:, :k].copy()
    out = ~(d2[:, :k] <= np.float32(radius))
    idx[out] = np.broadcast_to(idx[:, :1], idx.shape)[out]
    return idx, raw, d2


def d2_64(pc, a, b):
    """float64 squared distances between points a (N,) / (N,k) and b of the fp32 cloud"""
    p = np.asarray(pc, np.float64)
    return ((p[a] - p[b]) ** 2).sum(-1)


def rigid_fit(S, mu1, mu2):
    """R = V diag(1, 1, det(V U^T)) U^T of S = U diag(s) V^T, t = mu2 - R mu1; the identity for a NaN in S (seg_loss.py:34-55)"""
    dt = S.dtype
    if np.isnan(S).any():
        return np.eye(3, dtype=dt), np.zeros(3, dt), np.full(3, np.nan, dt)
    U, s, Vt = np.linalg.svd(S)
    V = Vt.T
    det = np.linalg.det(V @ U.T)
    R = V @ np.diag(np.array([1.0, 1.0, det], dt)) @ U.T
    return R.astype(dt), (mu2 - R @ mu1).astype(dt), s


def segloss64(pc, flow, mask, idx=None, loss_norm=1, eps=1e-5, dtype=np.float64):
    """All three losses and their gradients w.r.t. mask (N,K) for ONE cloud.  idx (N,k) or None (no smoothness term).
    -> dict: dynamic, smooth, entropy, R (K,3,3), t (K,3), sv (K,3) singular values of S_k, pc_transformed (N,3), g_dynamic, g_smooth, g_entropy"""
    pc32 = np.asarray(pc, np.float32)
    pc2 = (pc32 + np.asarray(flow, np.float32)).astype(dtype)
    p = pc32.astype(dtype)
    m = np.asarray(mask, np.float32).astype(dtype)
    N, K = m.shape
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = m.sum(0)
        mu1 = (m.T @ p) / sm[:, None]
        mu2 = (m.T @ pc2) / sm[:, None]
        R = np.zeros((K, 3, 3), dtype); t = np.zeros((K, 3), dtype); sv = np.zeros((K, 3), dtype)
        for o in range(K):
            S = (p - mu1[o]).T @ (m[:, o, None] * (pc2 - mu2[o]))
            R[o], t[o], sv[o] = rigid_fit(S, mu1[o], mu2[o])
    T = np.einsum("kij,nj->kni", R, p) + t[:, None, :]
    q = (m.T[:, :, None] * T).sum(0)
    r = q - pc2
    nr = np.sqrt((r * r).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(nr[:, None] > 0, r / nr[:, None], 0)
    out.update(dynamic=nr.mean(dtype=dtype), R=R, t=t, sv=sv, pc_transformed=q, g_dynamic=np.einsum("ni,kni->nk", u, T) / dtype(N))
    e = dtype(np.float32(eps))
    lm = np.log(np.maximum(m, e))
    out.update(entropy=-(m * lm).sum(-1).mean(dtype=dtype), g_entropy=-(lm + (m > e)) / dtype(N))
    if idx is not None:
        idx = np.asarray(idx, np.int64)
        k = idx.shape[1]
        diff = m[:, None, :] - m[idx]
        if loss_norm == 1:
            nrm = np.abs(diff).sum(-1)
            ge = np.sign(diff)
        elif loss_norm == 2:
            nrm = np.sqrt((diff * diff).sum(-1))
            with np.errstate(invalid="ignore", divide="ignore"):
                ge = np.where(nrm[..., None] > 0, diff / nrm[..., None], 0)
        else:
            raise ValueError("loss_norm must be 1 or 2")
        ge = ge / dtype(N * k)
        g = ge.sum(1)
        np.subtract.at(g, idx.reshape(-1), ge.reshape(-1, K))
        out.update(smooth=nrm.mean(dtype=dtype), g_smooth=g)
    return out


def idx_mismatch(pc, radius, got, ref, band=1e-5, points=None):
    """Rows where two neighbour tables differ, split into rows inside the near-tie band and rows outside it.  A slot counts with the float64
    squared distance of its neighbour, a replaced slot (the index of slot 0 in a later slot) with `radius`; a row is inside the band when every
    slot of `got` is within `band` (relative) of the same slot of `ref`.  points: the point of every row (default: row number).
    -> (n_differ, n_outside_band)"""
    got, ref = np.asarray(got, np.int64), np.asarray(ref, np.int64)
    rows = np.nonzero((got != ref).any(1))[0]
    if not rows.size:
        return 0, 0
    pts = rows if points is None else np.asarray(points, np.int64)[rows]

    def val(tab):
        t = tab[rows]
        v = d2_64(pc, pts[:, None], t)
        repl = np.zeros_like(t, bool)
        repl[:, 1:] = t[:, 1:] == t[:, :1]
        return np.where(repl, float(np.float32(radius)), v)

    a, b = val(got), val(ref)
    ok = (np.abs(a - b) <= band * np.abs(b) + 1e-30).all(1)
    return int(rows.size), int((~ok).sum())
