"""2-D mask supervision of a render (include/nvfi_hip.h: nvfi_mask_loss_fwd / nvfi_mask_loss_bwd; csrc/maskloss.hip).  The reference renders the
soft label map of a MaskField (tensorf_keyframe.py:749-753) but has no loss on it; the definition follows nvfi_render_mask on the samples of
the render that is supervised:

    q[r][k] = sum_{j in M_r} w_j softmax(MaskField(x_j))_k       x_j the warped keyframe position of masked sample j, w_j the render's weight
    loss    = 1 / (2 n K) sum_{valid r} sum_k (q_rk - y_rk)^2                     ("l2")
            = -(1 / n)    sum_{valid r} sum_k y_rk log(q_rk + eps)                ("ce")

y_r is one-hot for an int label in [0, K), zero for the label K (background), the row of a float (R, K) target; a negative label or a row with
a non-finite entry leaves the ray out, n counts the others.

This module holds the raw calls - one forward, one chunked backward - and the plan of their workspace.  The autograd form is
TensorVMKeyframeTimeKplane.mask_loss (NVFi.mask_loss), the fused-driver forms render_mse_backward_(..., target_mask=) and mask_fit_backward_."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr

KINDS = {"l2": 0, "ce": 1}


def mask_loss_plan(desc, mdesc, R, max_workspace_bytes=1 << 30):
    """(chunk_cap, workspace bytes, number of chunks) of a mask-loss call on R rays: the masked list has room for R * n_samples entries; the
    backward handles chunk_cap of them per call, the largest multiple of 128 whose plan stays under max_workspace_bytes (the MaskField's stash is
    ~4.4 KB per entry, on top of 148 bytes per entry of the capacity and 84 MB of weight-gradient slabs)."""
    L = _lib.lib()
    cap = -(-int(R) * int(desc.n_samples) // 128) * 128           # whole 128-entry workgroups

    def nbytes(n):
        return _lib.bytes_of(L.nvfi_mask_loss_workspace_bytes, C.byref(desc), C.byref(mdesc), R, n)

    return _lib.plan_chunks(nbytes, cap, max_workspace_bytes, "mask loss")


def mask_target(target, R, K):
    """(labels, soft) of a target as the library wants it: an integer tensor (R) -> contiguous int32 labels, a floating one (R, K) -> contiguous
    float32 rows.  A tensor that already has that form is passed through without a launch."""
    if not (isinstance(target, torch.Tensor) and target.is_cuda):
        raise _lib.NvfiError("NVFi HIP kernels need the mask target on the GPU (no CPU fallback exists)")
    if target.dtype.is_floating_point:
        if target.dim() != 2 or tuple(target.shape) != (R, K):
            raise ValueError(f"a float mask target must be (R, K) = ({R}, {K}), got {tuple(target.shape)}")
        return None, target.float().contiguous()
    if target.dtype == torch.bool or target.numel() != R:
        raise ValueError(f"an integer mask target must hold one label per ray ({R}), got {tuple(target.shape)} of {target.dtype}")
    return target.reshape(-1).to(torch.int32).contiguous(), None


def mask_loss_raw(desc, mdesc, render_ws, flags, weights, t, target, kind="ce", eps=1e-5, grad_scale=1.0, grad_scale_dev=None, g_weights=None,
                  add_gw=False, loss=None, mask_map=None, max_workspace_bytes=1 << 30, plan=None, workspace=None):
    """One nvfi_mask_loss_fwd call behind the render that filled `render_ws` (same desc, t, flags; `weights` its (R, S) output), nothing else ->
    dict(loss, mask_map, g_weights, workspace, chunk_cap, chunks, R, S).  loss: float32[2] device tensor (UN-scaled loss, n); mask_map (R, K);
    g_weights (R, S) = grad_scale [* grad_scale_dev] * d loss / d weights, WRITTEN, or with add_gw=True ADDED to the tensor given.  An output
    passed as False is left out of the call.  The workspace carries what mask_loss_backward_raw needs: keep it until then (`workspace`: a uint8
    tensor to use instead of a fresh one).  One library call and no torch launch when `target` arrives ready: contiguous int32 (R) labels or
    contiguous float32 (R, K) rows; anything else is converted here first with a torch launch, which a captured graph must not contain."""
    for x in (render_ws, weights):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    R, S = weights.shape
    K = int(mdesc.mask_dim)
    dev = weights.device
    t = float(np.float32(float(t)))
    labels, soft = mask_target(target, R, K)
    chunk, nbytes, chunks = plan if plan is not None else mask_loss_plan(desc, mdesc, R, max_workspace_bytes)
    if workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_cuda or workspace.numel() < nbytes):
        raise ValueError(f"workspace must be a uint8 device tensor of at least {nbytes} bytes (mask_loss_plan)")
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if loss is None:
        loss = torch.empty(2, device=dev)
    if mask_map is None:
        mask_map = torch.empty(R, K, device=dev)
    if g_weights is None:
        g_weights = torch.empty(R, S, device=dev)
    loss, mask_map, g_weights = (None if o is False else o for o in (loss, mask_map, g_weights))
    if add_gw and g_weights is None:
        raise ValueError("add_gw=True needs the g_weights tensor to add to")
    _lib.check(_lib.lib().nvfi_mask_loss_fwd(
        C.byref(desc), C.byref(mdesc), R, t, int(flags), _lib.ptr(weights), _lib.ptr(labels), _lib.ptr(soft),
        KINDS[kind], float(eps), float(grad_scale), _lib.ptr(grad_scale_dev),
        _lib.NVFI_MASKLOSS_ADD_GW if add_gw else 0, _lib.ptr(loss), _lib.ptr(mask_map), _lib.ptr(g_weights),
        _lib.ptr(render_ws), render_ws.numel(), chunk, _lib.ptr(ws), ws.numel(), _stream_ptr()))
    return dict(loss=loss, mask_map=mask_map, g_weights=g_weights, workspace=ws, chunk_cap=chunk, chunks=chunks, R=R, S=S, target=(labels, soft))


def mask_grads_struct(grads):
    """nvfi_mask_grads over ten tensors in MaskField._params() order (W0, b0, ..., W4, b4); None skips a tensor"""
    mg = _lib.MaskGrads()
    for i in range(5):
        mg.W[i] = _lib.ptr(grads[2 * i]); mg.b[i] = _lib.ptr(grads[2 * i + 1])
    return mg


def mask_loss_backward_raw(mdesc, call, MG):
    """The chunked nvfi_mask_loss_bwd of a mask_loss_raw result: the gradients of the ten MaskField tensors ACCUMULATED into the nvfi_mask_grads
    struct MG.  Chunks beyond the masked count launch kernels that exit at once: the count never reaches the host."""
    L = _lib.lib()
    ws, chunk = call["workspace"], call["chunk_cap"]
    for k in range(call["chunks"]):
        _lib.check(L.nvfi_mask_loss_bwd(C.byref(mdesc), call["R"], call["S"], k * chunk, chunk,
                                        C.byref(MG), _lib.ptr(ws), ws.numel(), _stream_ptr()))
