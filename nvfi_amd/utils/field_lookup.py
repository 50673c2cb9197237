"""Differentiable field lookups at given points (include/nvfi_hip.h: nvfi_density_grad, nvfi_appfeat_at, nvfi_appfeat_grad; csrc/lookup.hip):
the reference's compute_densityfeature / compute_appfeature (models/tensorf_keyframe.py:233-310) as autograd carries them to the planes, to
basis_mat.weight and to the points (x, y, z and the normalised time t').

This module holds the raw calls, one library call each and nothing else.  The autograd forms are TensorVMKeyframeTimeKplane.lookup_density /
lookup_appfeature (NVFi.lookup_density / lookup_appfeature); the density forward is nvfi_density_at (compute_densityfeature).

Beside them the raw call of differentiable point shading (nvfi_render_mlp_grad; csrc/point_shade.hip): render_mlp_grad_raw, the adjoint of
renderModule(pts, viewdirs, features); its autograd forms are field.shade / field.lookup_rgb."""
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
    _lib.check(_lib.lib().nvfi_density_grad(C.byref(desc), q.shape[0], _lib.ptr(q), _lib.ptr(g), _lib.ptr(out),
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
    _lib.check(_lib.lib().nvfi_appfeat_at(C.byref(desc), q.shape[0], _lib.ptr(q), _lib.ptr(out), _stream_ptr()))
    return out


def appfeat_grad_raw(desc, xyzt, g_feat, g_xyzt=True, grads=None):
    """One nvfi_appfeat_grad call: xyzt (N,4), g_feat (N, app_dim) -> g_xyzt (N,4) as in density_grad_raw.  grads: an _lib.Grads whose aps / apt /
    basis members are ACCUMULATED into (NULL members skipped), or None."""
    q = _points(xyzt)
    g = _upstream(g_feat, (q.shape[0], int(desc.app_dim)))
    out = _coord_out(g_xyzt, q)
    _lib.check(_lib.lib().nvfi_appfeat_grad(C.byref(desc), q.shape[0], _lib.ptr(q), _lib.ptr(g), _lib.ptr(out),
                                            None if grads is None else C.byref(grads), _stream_ptr()))
    return out


def _out(want, shape, like, name):
    """True: a fresh tensor of `shape`; a tensor: written in place; None / False: the call skips that output"""
    if want is True:
        return torch.empty(shape, device=like.device)
    if want is None or want is False:
        return None
    if not want.is_cuda or want.dtype != torch.float32 or not want.is_contiguous() or tuple(want.shape) != tuple(shape):
        raise ValueError(f"{name}: a contiguous float32 device tensor of shape {tuple(shape)} expected")
    return want


def render_mlp_grad_workspace_bytes(desc, n):
    return _lib.bytes_of(_lib.lib().nvfi_render_mlp_grad_workspace_bytes, C.byref(desc), n)


def render_mlp_grad_raw(desc, xyz, view, features, g_rgb, g_features=True, g_xyz=True, g_view=None, grads=None, workspace=None):
    """One nvfi_render_mlp_grad call (csrc/point_shade.hip), the adjoint of rgb = renderModule(xyz, view, features): xyz (N,3), view (N,3),
    features (N, app_dim), g_rgb (N,3) = d loss / d rgb -> (g_features, g_xyz, g_view), each OVERWRITTEN (True: a new tensor; a tensor: that
    one; None: skipped).  grads: an _lib.Grads whose rW / rb members are ACCUMULATED into buffers the caller cleared (NULL members skipped), or
    None.  workspace: a uint8 device tensor of at least render_mlp_grad_workspace_bytes(desc, N) bytes, or None (allocated here)."""
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda and view.is_cuda and features.is_cuda):
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    x = xyz.detach().reshape(-1, 3).contiguous().float()
    n, d = x.shape[0], int(desc.app_dim)
    v = view.detach().reshape(-1, 3).contiguous().float()
    fe = features.detach().reshape(-1, d).contiguous().float()
    if v.shape[0] != n or fe.shape[0] != n:
        raise ValueError(f"{n} points, {v.shape[0]} view directions, {fe.shape[0]} feature rows")
    g = _upstream(g_rgb, (n, 3))
    gf, gx, gv = _out(g_features, (n, d), x, "g_features"), _out(g_xyz, (n, 3), x, "g_xyz"), _out(g_view, (n, 3), x, "g_view")
    if workspace is None:
        workspace = torch.empty(render_mlp_grad_workspace_bytes(desc, n), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().nvfi_render_mlp_grad(C.byref(desc), n, _lib.ptr(x), _lib.ptr(v), _lib.ptr(fe), _lib.ptr(g), _lib.ptr(gf),
                                               _lib.ptr(gx), _lib.ptr(gv), None if grads is None else C.byref(grads), _lib.ptr(workspace),
                                               workspace.numel(), _stream_ptr()))
    return gf, gx, gv
