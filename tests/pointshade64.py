"""Float64 restatement, with autograd, of differentiable point shading (include/nvfi_hip.h: nvfi_render_mlp_grad; field.shade / lookup_rgb;
reference MLPRender_PE.forward, models/tensorf_base.py:88-98, and SHRender, models/tensorf_model_utils.py:292-296 + models/sh.py, under autograd):
the yardstick of tests/test_pointshade_golden.py (against the reference's goldens) and of tests/test_gpu_pointshade.py (against the device).

The statement is point64._render_module (the one mlp64 evaluates) with its inputs and parameters as autograd leaves; the loss is sum(rgb * g).  As
in the other yardsticks the inputs stay fp32-rounded and are then promoted; dtype=float32 is a plain fp32 implementation of the same statement, the
floor the bounds are derived from.  The one deliberately wrong variant is point64's `wrong=True`: the view encoding's highest frequency dropped
(MLP_PE), b[6] of the SH basis with zz - xx - yy (an SH field).

The discrete decisions of the statement are the ReLUs: 256 hidden units per point (MLP_PE), three clamps per point (SH).  A gradient is only
comparable where the float64 run, the float32 run and the device take the same decision, so the seeds of the test cases are chosen such that they
do, with room (`relu_margin`; tests/test_pointshade_golden.py checks every seed the GPU file uses): no point is masked out of any comparison."""
import numpy as np
import torch
import torch.nn.functional as F

import lookup64 as l64
import point64 as p64
import render64 as r64

MLP_NAMES = list(r64.MLP_NAMES)
bound = l64.bound
max_err = l64.max_err
MARGIN = 64.0          # the smallest |pre-activation| of a case is at least this many times that pre-activation's own |float32 - float64|


def app_dim(field):
    return 27 if field.sh else 32


def inputs(field, N, seed):
    """(xyz (N,3) in the box, view (N,3) unit vectors, features (N, app_dim), g_rgb (N,3)) float32, from one seed"""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((N, 3)) * 2 - 1).astype(np.float32)
    v = rng.standard_normal((N, 3))
    view = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    feat = (0.5 * rng.standard_normal((N, app_dim(field)))).astype(np.float32)
    g = rng.standard_normal((N, 3)).astype(np.float32)
    return xyz, view, feat, g


def _leaves(field, xyz, view, feat, dtype, device):
    P = {} if field.sh else {k: field.p32[k].to(device=device, dtype=dtype).requires_grad_(True) for k in MLP_NAMES}
    x = p64._t32(xyz, 3).to(device=device, dtype=dtype).requires_grad_(True)
    v = p64._t32(view, 3).to(device=device, dtype=dtype).requires_grad_(True)
    fe = p64._t32(feat, app_dim(field)).to(device=device, dtype=dtype).requires_grad_(True)
    return P, x, v, fe


def shade64(field, xyz, view, feat, g=None, dtype=torch.float64, device="cpu", wrong=False):
    """dict: rgb (N,3), and with g (N,3) = d loss / d rgb: g_features (N, app_dim), g_xyz (N,3), g_view (N,3), grads {name: array} of the six
    tensors of renderModule.mlp (empty for an SH field)"""
    P, x, v, fe = _leaves(field, xyz, view, feat, dtype, device)
    rgb = p64._render_module(field, P, x, v, fe, wrong)
    out = dict(rgb=rgb.detach().cpu().numpy())
    if g is not None:
        gt = p64._t32(g, 3).to(device=device, dtype=dtype)
        leaves = [fe, x, v] + [P[k] for k in P]
        grads = torch.autograd.grad((rgb * gt).sum(), leaves, allow_unused=True)
        grads = [(torch.zeros_like(a) if gr is None else gr).cpu().numpy() for a, gr in zip(leaves, grads)]
        out["g_features"], out["g_xyz"], out["g_view"] = grads[:3]
        out["grads"] = dict(zip(P, grads[3:]))
    return out


def tensors(y):
    """{label: array} of a result: rgb, the three per-point gradients and every parameter gradient"""
    out = {"rgb": y["rgb"]}
    if "g_features" in y:
        out.update({k: y[k] for k in ("g_features", "g_xyz", "g_view")})
        out.update({"grad:" + k: v for k, v in y["grads"].items()})
    return out


def preacts(field, xyz, view, feat, dtype=torch.float64, device="cpu"):
    """the arguments of every ReLU of the statement: [z1 (N,128), z2 (N,128)] (MLP_PE) or [sum + 0.5 (N,3)] (SH), numpy in `dtype`"""
    with torch.no_grad():
        P, x, v, fe = _leaves(field, xyz, view, feat, dtype, device)
        if field.sh:
            C0, C1 = 0.28209479177387814, 0.4886025119029199
            C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
            a, b, c = v[:, 0], v[:, 1], v[:, 2]
            bs = torch.stack([torch.full_like(a, C0), -C1 * b, C1 * c, -C1 * a, C2[0] * a * b, C2[1] * b * c, C2[2] * (2.0 * c * c - a * a - b * b),
                              C2[3] * a * c, C2[4] * (a * a - b * b)], 1)
            return [((bs[:, None, :] * fe.view(-1, 3, 9)).sum(-1) + 0.5).cpu().numpy()]
        h = torch.cat([fe, v, x, r64._pe(x, 6), r64._pe(v, 6)], -1)
        z1 = F.linear(h, P["renderModule.mlp.0.weight"], P["renderModule.mlp.0.bias"])
        z2 = F.linear(torch.relu(z1), P["renderModule.mlp.2.weight"], P["renderModule.mlp.2.bias"])
        return [z1.cpu().numpy(), z2.cpu().numpy()]


def relu_margin(field, xyz, view, feat, device="cpu"):
    """(same decisions, smallest |z64| / (MARGIN x |z32 - z64|) over every ReLU argument of the case): the case is usable when the first is true
    and the second is at least 1.  A pre-activation the two runs agree on exactly imposes nothing."""
    z64 = preacts(field, xyz, view, feat, torch.float64, device)
    z32 = preacts(field, xyz, view, feat, torch.float32, device)
    same, room = True, np.inf
    for a, b in zip(z64, z32):
        b = b.astype(np.float64)
        same = same and bool(((a > 0) == (b > 0)).all())
        d = MARGIN * np.abs(b - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d > 0, np.abs(a) / d, np.inf)
        room = min(room, float(r.min()))
    return same, room
