"""Float64 restatement of the PDE regulariser (reference models/nvfi.py:42-84, get_vel_loss) on a GIVEN kept set: the yardstick of
tests/test_pde64_golden.py (against the reference's goldens) and tests/test_gpu_pde64.py (against the device kernels).

The velocity net is written out here from the reference's VelBasis (models/velocity_field.py:54-98, mirrored by
nvfi_amd/models/velocity_field.py): the 28-wide encoder [q, sin(q), cos(q), sin(2q), cos(2q), sin(4q), cos(4q)] of q = (x, y, z, t),
weight_net (five SiLU layers) and a_weight_net (five ReLU layers) of width 128 with 6 outputs each, and the basis products
    v = (w0 - w4 z + w5 y,  w1 + w3 z - w5 x,  w2 - w3 y + w4 x)
    a = (a0 - (a4 + a5) x,  a1 - (a3 + a5) y,  a2 - (a3 + a4) z).
The Jacobian d(v, a) / d(x, y, z, t) comes from torch.func (forward mode, vmapped over the points), the gradients of the 24 parameters from
autograd through it, all in float64.  The loss is 5 mean(div^2) + 0.1 mean(transport^2) with div = tr J[:3, :3] and
transport = J[:3, :3] v + J[:3, 3] - a (mean over the 3 components too).  Kept points are processed in chunks and the sums accumulate in
float64, so half a million points fit in a few GB.

Parameters come in the order of TensorVMKeyframeTimeKplane._pde_params(): (weight, bias) of the six linears of weight_net, then of a_weight_net."""
import numpy as np
import torch

LINEAR_IDS = ["1", "3.0", "4.0", "5.0", "6.0", "7.0"]
NAMES = [f"vel_net.{net}.{i}.{wb}" for net in ("weight_net", "a_weight_net") for i in LINEAR_IDS for wb in ("weight", "bias")]
DIV_W, TR_W = 5.0, 0.1


def normalize_points(points, aabb):
    """world -> [-1, 1]^3 as get_vel_loss does it (nvfi.normalize_coord, tensorf_base.py: (p - aabb0) * (2 / size) - 1), in fp32 like the reference;
    the time coordinate enters the net unnormalised"""
    p = torch.as_tensor(np.asarray(points, np.float32)).reshape(-1, 3)
    a = torch.as_tensor(np.asarray(aabb, np.float32)).reshape(2, 3)
    inv = 2.0 / (a[1] - a[0])
    return (p - a[0]) * inv - 1.0


def _mlp(q, Ws, bs, act):
    enc = [q]
    for k in range(3):
        enc += [torch.sin(q * 2.0 ** k), torch.cos(q * 2.0 ** k)]
    h = torch.cat(enc, -1)
    for i in range(6):
        h = torch.nn.functional.linear(h, Ws[i], bs[i])
        if i < 5:
            h = act(h)
    return h


def vel_acc(q, params):
    """(v, a) of one point q = (x, y, z, t), float64: VelBasis.forward"""
    w = _mlp(q, params[0:12:2], params[1:12:2], torch.nn.functional.silu)
    aw = _mlp(q, params[12:24:2], params[13:24:2], torch.relu)
    x, y, z = q[0], q[1], q[2]
    v = torch.stack([w[0] - w[4] * z + w[5] * y, w[1] + w[3] * z - w[5] * x, w[2] - w[3] * y + w[4] * x])
    a = torch.stack([aw[0] - (aw[4] + aw[5]) * x, aw[1] - (aw[3] + aw[5]) * y, aw[2] - (aw[3] + aw[4]) * z])
    u = torch.cat([v, a])
    return u, u


def _chunk_terms(q, params):
    """per-point div^2 and |transport|^2 (each (n,)) and the Jacobian rows 0-2 ((n, 3, 4)) of the kept points q (n, 4)"""
    from torch.func import jacfwd, vmap
    jac, u = vmap(jacfwd(lambda p: vel_acc(p, params), has_aux=True))(q)
    J = jac[:, :3, :]
    v, a = u[:, :3], u[:, 3:]
    div = J[:, 0, 0] + J[:, 1, 1] + J[:, 2, 2]
    tr = torch.einsum("noi,ni->no", J[:, :, :3], v) + J[:, :, 3] - a
    return div * div, (tr * tr).sum(-1), J


def as_params(tensors, device="cpu", dtype=torch.float64):
    return [torch.as_tensor(np.asarray(p) if not isinstance(p, torch.Tensor) else p.detach().cpu()).to(device=device, dtype=dtype)
            for p in tensors]


def pde_sums(xn, t, params, idx=None, n_jac=0, grads=True, chunk=32768, acc_dtype=torch.float64):
    """UN-normalised sums over the points `idx` (default: all rows) of xn (P, 3) normalised coordinates and t (P,):
    S = 5 sum(div^2) + (0.1 / 3) sum(|transport|^2), sum(div^2), sum(|transport|^2), the gradients of S (24 float64 tensors) and the Jacobian
    rows 0-2 of the first n_jac points.  The PDE loss of a kept set of n points is S / n, its gradients dS / n.  The arithmetic runs in the
    parameters' dtype (as_params: float64; float32 is the plain fp32 evaluation of the same statement); the chunks are summed in acc_dtype."""
    device = params[0].device
    q_all = torch.cat([torch.as_tensor(xn).reshape(-1, 3), torch.as_tensor(t).reshape(-1, 1)], 1).to(device=device, dtype=params[0].dtype)
    if idx is not None:
        q_all = q_all[torch.as_tensor(np.asarray(idx), device=device, dtype=torch.long)]
    ps = [p.detach().clone().requires_grad_(grads) for p in params]
    g = [torch.zeros_like(p, dtype=acc_dtype) for p in ps]      # (acc_dtype float32: a plain fp32 sum over the chunks, one rounding per chunk)
    sd = st = 0.0
    jac = []
    for s in range(0, q_all.shape[0], chunk):
        with torch.set_grad_enabled(grads):
            d2, t2, J = _chunk_terms(q_all[s:s + chunk], ps)
            a, b = d2.sum(), t2.sum()
            if grads:
                for acc, gi in zip(g, torch.autograd.grad(DIV_W * a + TR_W / 3.0 * b, ps)):
                    acc += gi.to(acc_dtype)
        sd += float(a.detach()); st += float(b.detach())
        if s < n_jac:
            jac.append(J[: n_jac - s].detach())
    jac = torch.cat(jac).cpu().numpy() if jac else np.zeros((0, 3, 4))
    return dict(S=DIV_W * sd + TR_W / 3.0 * st, sum_div2=sd, sum_tr2=st, grads=[x.to(torch.float64).cpu().numpy() for x in g] if grads else None, jac=jac,
                n=int(q_all.shape[0]))


def pde64(points, t, kept, params, aabb, n_jac=0, grads=True, chunk=32768, acc_dtype=torch.float64):
    """get_vel_loss in float64 on the kept set `kept` (bool (P,)) of world-space points (P, 3) and raw times (P,) / (P, 1).
    params: the 24 tensors (any device; the arithmetic runs on params[0]'s device after conversion, see as_params).
    Returns dict(loss, n_kept, jac (n_jac, 3, 4), grads: {name: float64 array}, sums: pde_sums of the kept set)."""
    xn = normalize_points(points, aabb)
    t = torch.as_tensor(np.asarray(t, np.float32)).reshape(-1)
    idx = np.nonzero(np.asarray(kept).reshape(-1))[0]
    n = len(idx)
    if n == 0:
        return dict(loss=0.0, n_kept=0, jac=np.zeros((0, 3, 4)), grads=None, sums=None, xn=xn, t=t, idx=idx)
    s = pde_sums(xn, t, params, idx, n_jac, grads, chunk, acc_dtype)
    out = dict(loss=s["S"] / n, n_kept=n, jac=s["jac"], sums=s, xn=xn, t=t, idx=idx)
    out["grads"] = {k: gk / n for k, gk in zip(NAMES, s["grads"])} if grads else None
    return out


def without(ref, params, drop):
    """the float64 reference `ref` (a pde64 result) recomputed with the kept points at positions `drop` (indices into the kept list, e.g. one
    32-point tile) removed: from the full sums minus the sums of the dropped points, exact up to float64 rounding.  Returns (loss, grads)."""
    d = pde_sums(ref["xn"], ref["t"], params, ref["idx"][np.asarray(drop)], 0, True)
    n = ref["n_kept"] - len(drop)
    full = ref["sums"]
    return (full["S"] - d["S"]) / n, {k: (a - b) / n for k, a, b in zip(NAMES, full["grads"], d["grads"])}


def relu_margin(xn, t, params, chunk=32768):
    """per point, the smallest |z| / (fp32 rounding bound of z) over the hidden units of a_weight_net, in float64.  Below ~1 an fp32 evaluation may
    take the other side of a ReLU kink than float64, and the point's parameter gradient jumps there (the loss is continuous, its gradient is not)"""
    q_all = torch.cat([torch.as_tensor(xn).reshape(-1, 3), torch.as_tensor(t).reshape(-1, 1)], 1).to(device=params[0].device, dtype=torch.float64)
    out = []
    for s in range(0, q_all.shape[0], chunk):
        q = q_all[s:s + chunk]
        h = torch.cat([q] + [f(q * 2.0 ** k) for k in range(3) for f in (torch.sin, torch.cos)], 1)
        m = torch.full((q.shape[0],), float("inf"), dtype=torch.float64, device=q.device)
        for i in range(5):
            W, b = params[12 + 2 * i], params[13 + 2 * i]
            z = torch.nn.functional.linear(h, W, b)
            err = (torch.nn.functional.linear(h.abs(), W.abs()) + b.abs()) * (2.0 ** -24 * h.shape[1])
            m = torch.minimum(m, (z.abs() / err).min(1).values)
            h = torch.relu(z)
        out.append(m.cpu())
    return torch.cat(out).numpy()


def shift(ref, params, drop, metric):
    """largest metric(moved gradient, reference gradient) over the 24 tensors when the kept points `drop` are removed, and the loss's relative move"""
    loss, g = without(ref, params, drop)
    return max(metric(g[k], ref["grads"][k]) for k in NAMES), abs(loss - ref["loss"]) / abs(ref["loss"])
