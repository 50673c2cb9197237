"""Differentiable field lookups at given points (include/nvfi_hip.h: nvfi_density_grad, nvfi_appfeat_at, nvfi_appfeat_grad; csrc/lookup.hip):
the reference's compute_densityfeature / compute_appfeature (models/tensorf_keyframe.py:233-310) as autograd carries them to the planes, to
basis_mat.weight and to the points (x, y, z and the normalised time t').

This module holds the raw calls, one launch each and nothing else.  The autograd forms are TensorVMKeyframeTimeKplane.lookup_density /
lookup_appfeature (NVFi.lookup_density / lookup_appfeature); the density forward is nvfi_density_at (compute_densityfeature)."""
import ctypes as C

import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr


def _points(xyzt):
    if not (isinstance(xyzt, torch.Tensor) and xyzt.is_cuda):
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    return xyzt.detach().reshape(-1, 4).contiguous().float()


def _upstream(g, shape):
    if not g.is_cuda:
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    return g.detach().reshape(shape).contiguous().float()


def _coord_out(g_xyzt, q):
    """True: a fresh (N,4) tensor; a tensor: written in place; None / False: the call skips the coordinate gradient"""
    if g_xyzt is True:
        return torch.empty_like(q)
    if g_xyzt is None or g_xyzt is False:
        return None
    if not g_xyzt.is_cuda or g_xyzt.dtype != torch.float32 or not g_xyzt.is_contiguous() or tuple(g_xyzt.shape) != tuple(q.shape):
        raise ValueError(f"g_xyzt: a contiguous float32 device tensor of shape {tuple(q.shape)} expected")
    return g_xyzt


def density_grad_raw(desc, xyzt, g_feat, g_xyzt=True, grads=None):
    """One nvfi_density_grad call: xyzt (N,4), g_feat (N) or (N,1) = d loss / d feat -> g_xyzt (N,4), OVERWRITTEN (True: a new tensor; a tensor:
    that one; None: skipped).  grads: an _lib.Grads whose dps / dpt members are ACCUMULATED into (NULL members skipped), or None."""
    q = _points(xyzt)
    g = _upstream(g_feat, (q.shape[0],))
    out = _coord_out(g_xyzt, q)
    _lib.check(_lib.lib().nvfi_density_grad(C.byref(desc), C.c_int64(q.shape[0]), _lib.ptr(q), _lib.ptr(g), _lib.ptr(out),
                                            None if grads is None else C.byref(grads), _stream_ptr()))
    return out


def appfeat_raw(desc, xyzt, out=None):
    """One nvfi_appfeat_at call: xyzt (N,4) -> feat (N, app_dim) (written into `out` when given)"""
    q = _points(xyzt)
    shape = (q.shape[0], int(desc.app_dim))
    if out is None:
        out = torch.empty(shape, device=q.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != shape:
        raise ValueError(f"out: a contiguous float32 device tensor of shape {shape} expected")
    _lib.check(_lib.lib().nvfi_appfeat_at(C.byref(desc), C.c_int64(q.shape[0]), _lib.ptr(q), _lib.ptr(out), _stream_ptr()))
    return out


def appfeat_grad_raw(desc, xyzt, g_feat, g_xyzt=True, grads=None):
    """One nvfi_appfeat_grad call: xyzt (N,4), g_feat (N, app_dim) -> g_xyzt (N,4) as in density_grad_raw.  grads: an _lib.Grads whose aps / apt /
    basis members are ACCUMULATED into (NULL members skipped), or None."""
    q = _points(xyzt)
    g = _upstream(g_feat, (q.shape[0], int(desc.app_dim)))
    out = _coord_out(g_xyzt, q)
    _lib.check(_lib.lib().nvfi_appfeat_grad(C.byref(desc), C.c_int64(q.shape[0]), _lib.ptr(q), _lib.ptr(g), _lib.ptr(out),
                                            None if grads is None else C.byref(grads), _stream_ptr()))
    return out
