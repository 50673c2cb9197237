"""Optical-flow supervision of a training render (include/nvfi_hip.h: nvfi_flow_loss_fwd / nvfi_flow_loss_bwd; csrc/flowloss.hip).  The reference
has no such term; the definition follows the eval-mode flow map of nvfi_render_flow on the samples of a TRAINING render:

    flow2d[r] = sum_{j in M_r} w_j (pi(Phi(x_j)) - pi(x_j)),   Phi = integrate_pos(., t, t + dt),   pi the pinhole projection of `camera`
    loss      = (1 / (2 n)) sum_{valid r} sum_c rho(flow2d[r][c] - target[r][c]),   rho(e) = e^2 ("l2") or torch's huber element ("huber")

This module holds the raw calls - one forward, one chunked backward - and the plan of their workspace.  The autograd form is
TensorVMKeyframeTimeKplane.flow_loss (NVFi.flow_loss), the fused-driver form render_mse_backward_(..., target_flow=)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr

KINDS = {"l2": 0, "huber": 1}


def flow_camera(camera, device):
    """(pose (3,4) fp32 device tensor, H, W, focal) of anything with pose / height / width / focal as models.Camera has them, or of a tuple
    (pose3x4, H, W, focal).  A pose that already lives on the device is not read on the host."""
    if camera is None:
        raise ValueError("the flow loss needs a camera: (pose3x4, H, W, focal) or an object with pose / height / width / focal")
    if isinstance(camera, (tuple, list)):
        pose, H, W, focal = camera
    else:
        pose, H, W, focal = camera.pose, camera.height, camera.width, camera.focal
    pose = torch.as_tensor(pose, dtype=torch.float32, device=device)[:3, :4].contiguous()
    return pose, int(H), int(W), float(focal)


def flow_loss_plan(desc, R, t, dt, max_workspace_bytes=1 << 30):
    """(chunk_cap, workspace bytes, number of chunks) of a flow-loss call on R rays: the masked list has room for R * n_samples entries; the
    backward handles chunk_cap of them per call, the largest multiple of 128 whose plan stays under max_workspace_bytes (the adjoint's stash is
    ~10.8 KB per entry and RK2 step).  Raises NvfiError (error 2) for what the library refuses: use_vel == 0, vel_fp16 1 / 2, more than 64 steps."""
    L = _lib.lib()
    cap = int(R) * int(desc.n_samples)

    def nbytes(n):
        return _lib.bytes_of(L.nvfi_flow_loss_workspace_bytes, C.byref(desc), R, t, dt, n)

    return _lib.plan_chunks(nbytes, cap, max_workspace_bytes, "flow loss")


def flow_loss_raw(desc, render_ws, flags, rays_o, rays_d, weights, t, dt, camera, target, valid=None, kind="l2", huber_delta=1.0,
                  grad_scale=1.0, grad_scale_dev=None, g_weights=None, add_gw=False, loss=None, flow2d=None, max_workspace_bytes=1 << 30,
                  plan=None):
    """One nvfi_flow_loss_fwd call behind the training render that filled `render_ws` (same desc, rays, t, flags; `weights` its (R, S) output),
    nothing else -> dict(loss, flow2d, g_weights, workspace, chunk_cap, chunks, R, t, dt).  loss: float32[2] device tensor (UN-scaled loss, n);
    flow2d (R, 2); g_weights (R, S) = grad_scale [* grad_scale_dev] * d loss / d weights, WRITTEN, or with add_gw=True ADDED to the tensor given.
    An output passed as False is left out of the call.  The workspace carries what flow_loss_backward_raw needs: keep it until then.
    The call itself is one library call and no torch launch when its inputs arrive ready: the pose a float32 device tensor, `target` a contiguous
    float32 (R, 2) device tensor and `valid` a contiguous uint8 device tensor.  Anything else is converted here first (a copy from the host for the
    pose, a torch launch for a bool / float mask or a non-float32 target), which a captured graph must not contain: convert once outside."""
    for x in (render_ws, rays_o, rays_d, weights, target):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    R, S = weights.shape
    dev = weights.device
    t, dt = float(np.float32(float(t))), float(np.float32(float(dt)))
    pose, H, W, focal = flow_camera(camera, dev)
    target = target.reshape(-1, 2).contiguous().float()
    if target.shape[0] != R:
        raise ValueError(f"target_flow must hold one (u, v) per ray ({R}), got {tuple(target.shape)}")
    if valid is not None:
        valid = valid.reshape(-1)
        if valid.numel() != R or not valid.is_cuda:
            raise ValueError(f"valid must be a device tensor with one entry per ray ({R})")
        valid = (valid != 0).to(torch.uint8).contiguous() if valid.dtype != torch.uint8 else valid.contiguous()
    chunk, nbytes, chunks = plan if plan is not None else flow_loss_plan(desc, R, t, dt, max_workspace_bytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if loss is None:
        loss = torch.empty(2, device=dev)
    if flow2d is None:
        flow2d = torch.empty(R, 2, device=dev)
    if g_weights is None:
        g_weights = torch.empty(R, S, device=dev)
    loss, flow2d, g_weights = (None if o is False else o for o in (loss, flow2d, g_weights))
    if add_gw and g_weights is None:
        raise ValueError("add_gw=True needs the g_weights tensor to add to")
    _lib.check(_lib.lib().nvfi_flow_loss_fwd(
        C.byref(desc), R, _lib.ptr(rays_o), _lib.ptr(rays_d), t, dt, int(flags), _lib.ptr(weights),
        _lib.ptr(pose), H, W, focal, _lib.ptr(target), _lib.ptr(valid), KINDS[kind], float(huber_delta),
        float(grad_scale), _lib.ptr(grad_scale_dev), _lib.NVFI_FLOWLOSS_ADD_GW if add_gw else 0,
        _lib.ptr(loss), _lib.ptr(flow2d), _lib.ptr(g_weights), _lib.ptr(render_ws), render_ws.numel(), chunk,
        _lib.ptr(ws), ws.numel(), _stream_ptr()))
    return dict(loss=loss, flow2d=flow2d, g_weights=g_weights, workspace=ws, chunk_cap=chunk, chunks=chunks, R=R, t=t, dt=dt)


def flow_loss_backward_raw(desc, call, G):
    """The chunked nvfi_flow_loss_bwd of a flow_loss_raw result: the gradient of weight_net ACCUMULATED into the nvfi_grads struct G (vW / vb; the
    rest is ignored).  Chunks beyond the masked count launch kernels that exit at once: the count never reaches the host."""
    L = _lib.lib()
    ws, chunk = call["workspace"], call["chunk_cap"]
    for k in range(call["chunks"]):
        _lib.check(L.nvfi_flow_loss_bwd(C.byref(desc), call["R"], call["t"], call["dt"], k * chunk,
                                        chunk, C.byref(G), _lib.ptr(ws), ws.numel(), _stream_ptr()))
