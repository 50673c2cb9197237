"""The losses of the reference's segmentation training (utils/seg_loss.py, called by train_segm.py:182-202) on the HIP kernels of
nvfi_amd/csrc/segloss.hip: same names and signatures, so `from utils.seg_loss import dynamic_loss, smooth_loss, entropy_loss` becomes
`from nvfi_amd.utils.seg_loss import ...` and the loss block runs unchanged.  No third-party package is needed (the reference's module imports
pytorch3d for the neighbour search; here that is nvfi_knn_self).

Every function is an autograd function over the C ABI (nvfi_knn_self / nvfi_segloss, include/nvfi_hip.h): forward and backward are ONE call,
the gradient w.r.t. `mask` is kept and scaled by the upstream gradient in backward.  Only `mask` receives a gradient: `pc` / `flow` that
require one raise NotImplementedError (train_segm.py computes both under no_grad).  There is no CPU path: CPU tensors raise NvfiError.
Inputs are (B, N, .) as in the reference; B = 1 is the hot path, B > 1 loops over the batch.  `segm_losses` is the fused form of a training
step: one neighbour search, one forward + backward for all three terms.

Behaviour kept from the reference, on purpose:
  * smooth_loss compares SQUARED neighbour distances with `radius` (seg_loss.py:96-98), so radius=0.01 is a ball of radius 0.1;
  * a neighbour slot beyond the radius is replaced by slot 0 - the point itself - and still counts in the mean (as a zero);
  * the rigid fit is detached (seg_loss.py:79): the gradient of dynamic_loss goes through the mask weights only, no SVD backward;
  * an object whose weighted moments contain a NaN (an all-zero mask column: 0 / 0) gets R = I, t = 0.
Differences: neighbours are ordered by (squared distance, index), a total order (pytorch3d leaves ties open); `pc_transformed` is returned
detached; rank_loss (unused by train_segm.py) is not provided; fit_motion_svd_batch forms pc2 as pc1 + (pc2 - pc1) in fp32."""

import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.NvfiError("the segmentation losses run on the GPU only (no CPU fallback exists)")


def _no_grad_inputs(**named):
    for name, t in named.items():
        if t is not None and t.requires_grad:
            raise NotImplementedError(f"`{name}` requires grad: only `mask` receives a gradient (train_segm.py computes {name} under no_grad)")


def _f32(t):
    return t.detach().contiguous().float()


def _workspace(N, K, k, device):
    nbytes = _lib.bytes_of(_lib.lib().nvfi_segloss_workspace_bytes, N, K, k)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def knn_self(pc, k, radius, reverse=True, return_dist=False):
    """pc (N,3) -> idx (N,k) int32 [, d2 (N,k)] and, with reverse, the reverse adjacency lists (rev_start (N+1), rev_edge (N*k)) that the
    smoothness gradient gathers through (see nvfi_knn_self in include/nvfi_hip.h for the ordering and the radius rule)."""
    _need_gpu(pc)
    if pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError("knn_self expects (N,3) points")
    pc = _f32(pc)
    N = pc.shape[0]
    idx = torch.empty(N, k, dtype=torch.int32, device=pc.device)
    d2 = torch.empty(N, k, dtype=torch.float32, device=pc.device) if return_dist else None
    rs = torch.empty(N + 1, dtype=torch.int32, device=pc.device) if reverse else None
    re = torch.empty(N * k, dtype=torch.int32, device=pc.device) if reverse else None
    ws = _workspace(N, 0, k, pc.device)
    with torch.cuda.device(pc.device):
        _lib.check(_lib.lib().nvfi_knn_self(N, _lib.ptr(pc), k, radius, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(rs),
                                            _lib.ptr(re), _lib.ptr(ws), ws.numel(), _stream_ptr()))
    return idx, d2, rs, re


class _SegLossFn(torch.autograd.Function):
    """autograd boundary around nvfi_segloss: (mask (N,K); pc, flow (N,3) or None; nn = (idx, rev_start, rev_edge) or None) ->
    (weighted total, losses (4), R (K,3,3), t (K,3), pc_transformed (N,3)); only the total is differentiable, and only w.r.t. mask."""

    @staticmethod
    def forward(ctx, mask, pc, flow, nn, k, loss_norm, eps, wd, ws_, we):
        N, K = mask.shape
        dev = mask.device
        m = _f32(mask)
        want_grad = ctx.needs_input_grad[0]
        g = torch.empty(N, K, dtype=torch.float32, device=dev) if want_grad else None
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        rigid = pc is not None
        R = torch.empty(K, 3, 3, dtype=torch.float32, device=dev) if rigid else None
        t = torch.empty(K, 3, dtype=torch.float32, device=dev) if rigid else None
        pct = torch.empty(N, 3, dtype=torch.float32, device=dev) if rigid else None
        idx, rs, re = nn if nn is not None else (None, None, None)
        ws = _workspace(N, K, k if nn is not None else 0, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nvfi_segloss(
                N, K, _lib.ptr(pc), _lib.ptr(flow), _lib.ptr(m), k, _lib.ptr(idx), _lib.ptr(rs), _lib.ptr(re),
                loss_norm, eps, wd, ws_, we, 1.0, 0,
                _lib.ptr(g), _lib.ptr(losses), _lib.ptr(R), _lib.ptr(t), _lib.ptr(pct), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        ctx.g = g
        ctx.mask_dtype = mask.dtype
        outs = (losses[3], losses, R, t, pct)
        ctx.mark_non_differentiable(*[o for o in outs[1:] if o is not None])
        return outs

    @staticmethod
    def backward(ctx, g_total, *unused):
        g = ctx.g
        if g is None:
            return (None,) * 10
        return ((g * g_total).to(ctx.mask_dtype),) + (None,) * 9


def _check_shapes(pc, mask, flow):
    if mask.dim() != 3:
        raise ValueError("mask must be (B, N, K)")
    B, N, K = mask.shape
    for name, t in (("pc", pc), ("flow", flow)):
        if t is not None and tuple(t.shape) != (B, N, 3):
            raise ValueError(f"{name} must be (B, N, 3) = {(B, N, 3)}, got {tuple(t.shape)}")
    if not 2 <= K <= 16:
        raise NotImplementedError("2..16 objects are supported")
    if N == 0:
        raise ValueError("no points")
    return B, N, K


def fit_motion_svd_batch(pc1, pc2, mask=None):
    """pc1, pc2 (B,N,3), mask (B,N) or None -> R (B,3,3), t (B,3): the weighted least-squares rigid motion pc1 -> pc2 (seg_loss.py:6-57);
    the identity for a batch entry whose moments contain a NaN.  No gradient."""
    _need_gpu(pc1, pc2, mask)
    if pc1.dim() != 3 or pc1.shape != pc2.shape or pc1.shape[2] != 3:
        raise ValueError("pc1, pc2 must be (B, N, 3)")
    B, N, _ = pc1.shape
    Rs, ts = [], []
    with torch.no_grad():
        for b in range(B):
            p1 = _f32(pc1[b])
            w = torch.zeros(N, 2, dtype=torch.float32, device=p1.device)      # object 0 carries the weights; object 1 is empty (identity, dropped)
            w[:, 0] = 1.0 if mask is None else _f32(mask[b])
            _, _, R, t, _ = _SegLossFn.apply(w, p1, _f32(pc2[b]) - p1, None, 0, 1, 1e-5, 1.0, 0.0, 0.0)
            Rs.append(R[0]); ts.append(t[0])
    return torch.stack(Rs), torch.stack(ts)


def _per_batch(fn, B):
    outs = [fn(b) for b in range(B)]
    return outs[0] if B == 1 else tuple(torch.stack(o) for o in zip(*outs))


def dynamic_loss(pc, mask, flow):
    """pc (B,N,3), mask (B,N,K), flow (B,N,3) -> (loss, pc_transformed (B,N,3)): mean ||sum_k m_k (R_k pc + t_k) - (pc + flow)||_2 with the
    per-object rigid fit of the mask-weighted points (seg_loss.py:60-86)."""
    _need_gpu(pc, mask, flow)
    _no_grad_inputs(pc=pc, flow=flow)
    B, N, K = _check_shapes(pc, mask, flow)
    res = [_SegLossFn.apply(mask[b], _f32(pc[b]), _f32(flow[b]), None, 0, 1, 1e-5, 1.0, 0.0, 0.0) for b in range(B)]
    loss = res[0][0] if B == 1 else torch.stack([r[0] for r in res]).mean()
    return loss, torch.stack([r[4] for r in res])


def smooth_loss(pc, mask, k=16, radius=0.1, loss_norm=1):
    """mean over (n, j) of ||mask[n] - mask[idx[n, j]]||_p over the k nearest points of the same cloud, slots whose SQUARED distance exceeds
    `radius` replaced by slot 0 (seg_loss.py:89-101).  loss_norm is 1 or 2."""
    _need_gpu(pc, mask)
    _no_grad_inputs(pc=pc)
    if loss_norm not in (1, 2):
        raise NotImplementedError("loss_norm must be 1 or 2")
    if not 1 <= int(k) <= 16:
        raise NotImplementedError("1..16 neighbours are supported")
    B, N, K = _check_shapes(pc, mask, None)
    res = []
    for b in range(B):
        idx, _, rs, re = knn_self(pc[b], int(k), float(radius), reverse=mask.requires_grad)
        res.append(_SegLossFn.apply(mask[b], None, None, (idx, rs, re), int(k), int(loss_norm), 1e-5, 0.0, 1.0, 0.0)[0])
    return res[0] if B == 1 else torch.stack(res).mean()


def entropy_loss(mask, epsilon=1e-5):
    """-mean_n sum_k m log(max(m, epsilon)) (seg_loss.py:104-112)."""
    _need_gpu(mask)
    _check_shapes(None, mask, None)
    K = mask.shape[-1]
    return _SegLossFn.apply(mask.reshape(-1, K), None, None, None, 0, 1, float(epsilon), 0.0, 0.0, 1.0)[0]


def segm_losses(pc, mask, flow, k, radius, smooth_w, entropy_w=0.0, loss_norm=1, epsilon=1e-5):
    """The objective of one training step in one pass: dynamic_loss + smooth_w * smooth_loss(k, radius) + entropy_w * entropy_loss with one
    neighbour search and one forward + backward call.  Returns (loss, parts): `loss` carries the gradient w.r.t. mask, `parts` is the
    detached (B, 3) tensor of the three un-weighted values (dynamic, smooth, entropy) for logging."""
    _need_gpu(pc, mask, flow)
    _no_grad_inputs(pc=pc, flow=flow)
    if loss_norm not in (1, 2):
        raise NotImplementedError("loss_norm must be 1 or 2")
    if not 1 <= int(k) <= 16:
        raise NotImplementedError("1..16 neighbours are supported")
    B, N, K = _check_shapes(pc, mask, flow)
    res = []
    for b in range(B):
        p = _f32(pc[b])
        idx, _, rs, re = knn_self(p, int(k), float(radius), reverse=mask.requires_grad)
        res.append(_SegLossFn.apply(mask[b], p, _f32(flow[b]), (idx, rs, re), int(k), int(loss_norm), float(epsilon), 1.0, float(smooth_w), float(entropy_w)))
    loss = res[0][0] if B == 1 else torch.stack([r[0] for r in res]).mean()
    return loss, torch.stack([r[1][:3] for r in res])
