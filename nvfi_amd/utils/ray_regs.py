"""Regularisers on the (R, S) ray weights of a training render.  The reference has none; the render backward takes their gradient as
`g_weights` (nvfi_render_bwd[_t]).

distortion loss (Mip-NeRF 360, Barron et al. 2022, eq. 15; as adopted by K-Planes, HexPlane, DVGO): penalises weight that is spread along a
ray - floaters and semi-transparent fog.  A ray's samples are equally spaced here (z_j = t_min + step (j + u) in every built sampling path), so
in normalised distance s = (z - near) / (far - near) every interval has the width delta = stepSize / (far - near), two midpoints differ by
(j - i) delta, and the loss of piecewise-constant intervals is

    D_r = delta [ sum_i sum_j w_i w_j |i - j| + (1/3) sum_i w_i^2 ],     loss = (1/R) sum_r D_r

csrc/raydist.hip forms the value and d loss / d weights in one kernel launch (+ one single-workgroup launch for the mean over rays)."""

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import stream_ptr as _stream_ptr


def distortion_workspace(R, device):
    """the workspace of one nvfi_ray_distortion call on R rays (uint8 device tensor)"""
    nbytes = _lib.bytes_of(_lib.lib().nvfi_ray_distortion_workspace_bytes, R)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def distortion_loss_raw(weights, delta, grad_scale=1.0, grad_scale_dev=None, out=None, want_per_ray=False, workspace=None):
    """One nvfi_ray_distortion call (include/nvfi_hip.h) on an (R, S) device tensor, nothing else: -> (loss, g_weights) or, with
    want_per_ray=True, (loss, g_weights, per_ray): a 0-dim tensor with the UN-scaled mean over rays, grad_scale [* grad_scale_dev] *
    d(loss)/d(weights) (R, S), and D_r per ray (R,).  grad_scale_dev: a device float tensor of one element that is multiplied into the
    gradient on the device (an upstream gradient: no host synchronisation).  out: the tensors to write into, in the order returned; an entry
    that is None is left out of the call (the kernel skips that output) and comes back as None.  workspace: distortion_workspace(R, device),
    for callers that keep one (hipGraph capture); it is needed, and allocated here if not given, only when `loss` is asked for.  Non-contiguous or non-fp32 weights are made contiguous fp32 first."""
    if not weights.is_cuda or (grad_scale_dev is not None and not grad_scale_dev.is_cuda):
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if weights.dim() != 2:
        raise ValueError(f"weights must be (R, S), got {tuple(weights.shape)}")
    if grad_scale_dev is not None and (grad_scale_dev.dtype != torch.float32 or grad_scale_dev.numel() != 1):
        raise ValueError("grad_scale_dev must be a float32 tensor of one element")
    weights = weights.detach().contiguous().float()
    R, S = weights.shape
    dev = weights.device
    if out is None:
        out = (torch.empty((), device=dev), torch.empty(R, S, device=dev)) + ((torch.empty(R, device=dev),) if want_per_ray else ())
    loss, g_w = out[0], out[1]
    per_ray = out[2] if len(out) > 2 else None
    for o, shape in ((loss, ()), (g_w, (R, S)), (per_ray, (R,))):
        if o is not None and (not o.is_cuda or o.dtype != torch.float32 or not o.is_contiguous() or tuple(o.shape) != shape):
            raise ValueError(f"out: a contiguous float32 device tensor of shape {shape} expected, got {tuple(o.shape)} {o.dtype}")
    if workspace is None and loss is not None:       # only the mean over rays uses it: a call without `loss` (the autograd backward) needs none
        workspace = distortion_workspace(R, dev)
    _lib.check(_lib.lib().nvfi_ray_distortion(R, S, _lib.ptr(weights), float(delta), float(grad_scale),
                                              _lib.ptr(grad_scale_dev), _lib.ptr(loss), _lib.ptr(per_ray), _lib.ptr(g_w),
                                              _lib.ptr(workspace), 0 if workspace is None else workspace.numel(), _stream_ptr()))
    return (loss, g_w, per_ray) if (want_per_ray or len(out) > 2) else (loss, g_w)


class _DistortionFn(torch.autograd.Function):
    """forward: the value only; backward: one launch that writes upstream * d(loss)/d(weights), the upstream gradient read on the device"""

    @staticmethod
    def forward(ctx, weights, delta):
        w = weights.detach().contiguous().float()
        loss = torch.empty((), device=w.device)
        distortion_loss_raw(w, delta, out=(loss, None))
        ctx.save_for_backward(w)
        ctx.delta, ctx.dtype = float(delta), weights.dtype
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        g_w = torch.empty_like(w)
        distortion_loss_raw(w, ctx.delta, grad_scale_dev=g.detach().reshape(1).contiguous().float(), out=(None, g_w))
        return g_w.to(ctx.dtype), None


def distortion_loss(weights, delta):
    """Distortion loss of the (R, S) ray weights of a training render (`out[3]` of the field's forward) with interval width `delta`
    (field.distortion_delta(): stepSize / (far - near)) -> 0-dim tensor, differentiable once with respect to `weights`.  The drop-in form
    `loss = mse + lam * distortion_loss(weights, field.distortion_delta())` costs two launches forward and one backward; the fused driver
    form is TensorVMKeyframeTimeKplane.render_mse_backward_(..., distortion_weight=lam).  There is no CPU path: CPU tensors raise NvfiError.
    Multi-GPU: every rank's mean is over its OWN shard of the batch."""
    if not weights.is_cuda:
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if weights.dim() != 2:
        raise ValueError(f"weights must be (R, S), got {tuple(weights.shape)}")
    return _DistortionFn.apply(weights, float(delta))
