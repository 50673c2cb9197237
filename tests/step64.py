"""Float64 yardstick of ONE training iteration of the reference's --static_dynamic loop (train_nvfi.py:139-249): the composition of the per-term
yardsticks, nothing restated a second time.

  total loss = mse(render(t1)) + mse(render(t_key)) + L1w L1 + tvd TVd + tva TVa + vw L_vel          (the last term only if a point is kept)
      the two renders and their MSE: render64.render64 with render64.Loss (optim64.mse on the fp32 colour map cross-checks the value);
      L1, TVd, TVa and their weighted gradient: optim64.regs;  L_vel on the GIVEN kept set: pde64.pde64;  the update: optim64.adam.
  schedule, from the iteration index `it` (0-based) alone - never read from a driver: every loss weight is multiplied by 0.1^(1/30000) BEFORE it is
      used (iteration `it` uses w0 f^(it+1); w0 = 8e-4, 1, 1, 1), the learning rates AFTER the step (iteration `it` steps with lr0 f^it; lr0 = 0.02 for
      the twelve planes, 1e-3 for everything else: get_optparam_groups(0.02, 1e-3)), Adam's step count is it + 1, betas (0.9, 0.99), eps 1e-8.
      The powers are formed as the drivers form them, by repeated multiplication in double.
  a radiance-only iteration (no velocity field) is the same statement with one render and no PDE term: `batches` holds one batch, `pde` is None.

`terms` evaluates what is expensive (the renders with their gradients, the PDE term with its gradients) at one set of parameters; `combine` adds
the regularisers, weighs the shares by the schedule, sums them and takes the Adam step.  `step64` is the two in a row.  With dtype = float32 every
piece runs as "a plain fp32 implementation of the same statement" (the chunks of rays and points and the shares are summed in float32 too: render64 /
pde64 get acc_dtype = dtype; `chunk` / `pde_chunk` set the length of those sums, and with it the order of the fp32 additions): its distance from the float64 run is the
rounding a correct fp32 iteration may show, the figure the tests derive their bounds from.  `free_run` iterates step64 on its own output; the
state (parameters and moments) is rounded to fp32 between iterations, as the reference stores it.

The deliberately wrong variants, computed only here (`variant=`), which the tests' bounds have to see:
  "a"  the loss weights decayed after use (iteration `it` uses w0 f^it)
  "b"  the learning rates decayed before the step (lr0 f^(it+1))
  "c"  Adam's bias corrections at t - 1 (at it = 0, where that is a division by zero, the right t is kept)
  "d"  the gradient of the previous iteration not cleared: g_k + g_(k-1)                               (needs g_prev)
  "e"  the gradient evaluated at the previous iteration's parameters - stale weight fragments -, applied to the current ones (needs stale terms)
  "f1" / "f2"  the PDE's / render 1's share missing from the velocity net (vel_net.weight_net.*; a lost chain of the three-stream step)
  "g"  the regularisers' share counted twice on the planes
kept64 decides the PDE term's kept set as get_vel_loss does (nvfi.py:49-64) from the existing pieces: point64.integrate64 back to the base keyframe
time, point64.density64 there, alpha = 1 - exp(-0.25 sigma) >= alphaMask_thres, the comparison on fp32 values."""
import numpy as np
import torch

import optim64
import pde64
import point64
import render64 as r64

LR_FACTOR = 0.1 ** (1 / 30000)
W0 = (8e-4, 1.0, 1.0, 1.0)                 # L1w, tvd, tva, vw
B1, B2, EPS = 0.9, 0.99, 1e-8
A_NAMES = pde64.NAMES[12:]
NAMES = r64.NAMES + A_NAMES                # the 43 tensors a term of the loss reaches
REG_NAMES = [f"{b}.{i}" for b in ("density_plane_space", "density_plane_time", "app_plane_space") for i in range(3)]
FAMILY = dict(r64.FAMILY, **{n: "vel" for n in A_NAMES})
FAMILIES = ("density", "app", "mlp", "vel")
VARIANTS = ("a", "b", "c", "d", "e", "f1", "f2", "g")


def lr0(name):
    return 0.02 if "plane" in name else 1e-3


def _decayed(x, n):
    for _ in range(n):
        x = x * LR_FACTOR
    return x


def schedule(it, variant=None):
    """what iteration `it` (0-based) uses, and what a driver holds after it: weights (L1w, tvd, tva, vw), lr(name), Adam's step count"""
    kw = it if variant == "a" else it + 1
    kl = it + 1 if variant == "b" else it
    return dict(w=tuple(_decayed(w, kw) for w in W0), lr_plane=_decayed(0.02, kl), lr_net=_decayed(1e-3, kl), step=it + 1,
                t_bias=max(it, 1) if variant == "c" else it + 1,
                after=dict(w=tuple(_decayed(w, it + 1) for w in W0), lr_plane=_decayed(0.02, it + 1), lr_net=_decayed(1e-3, it + 1), step=it + 1))


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def make_field(sd, meta):
    """point64.field_of (render64.Field + the acceleration net) plus the occupancy threshold of get_vel_loss; the parameters {name: fp32 array}"""
    f = point64.field_of(sd, meta)
    f.alpha_thres = float(meta["alphaMask_thres"])
    sd = {(k[5:] if k.startswith("nvfi.") else k): np.asarray(x) for k, x in sd.items()}
    return f, {k: np.asarray(sd[k], np.float32) for k in list(NAMES) + [n for n in ("basis_mat_density.weight",) if n in sd]}


def load(field, params):
    """the fp32 parameters {name: array} into a point64.field_of field (render64.Field + the acceleration net)"""
    for k in r64.NAMES:
        field.p32[k] = torch.from_numpy(np.ascontiguousarray(params[k], dtype=np.float32))
    field.a32 = {k: torch.from_numpy(np.ascontiguousarray(params[k], dtype=np.float32)) for k in A_NAMES if k in params}
    return field


def kept64(field, points, t, dtype=torch.float64, device="cpu"):
    """(kept (P,) bool, |alpha - thres| (P,)) of world-space points and raw times, by get_vel_loss's occupancy rule"""
    xn = pde64.normalize_points(points, field.aabb)
    t32 = torch.as_tensor(np.asarray(t, np.float32)).reshape(-1)
    scale = field.tmax / (field.K - 1)
    base = torch.round((t32 / scale).clamp(0.0, field.K - 1)) * scale
    xk = point64.integrate64(field, xn, t32, base, dtype=dtype, device=device)["xk"]
    tn = (base * 2 / field.tmax - 1).numpy()
    sigma = point64.density64(field, np.concatenate([xk.astype(np.float32), tn[:, None]], 1), dtype=dtype, device=device)["sigma"]
    # `1 - torch.exp(-sigma * 0.01 * 25)` on an fp32 tensor: exp(-x) near 1 sits on a grid of 6e-8, so alpha (~1e-4 at the threshold) does too, and
    # the decision is taken on THAT value; the float64 alpha says how far the point is from the threshold
    s32 = sigma.astype(np.float32)
    alpha32 = np.float32(1) - np.exp(((-s32) * np.float32(0.01)) * np.float32(25))
    alpha = 1.0 - np.exp(-sigma.astype(np.float64) * (0.01 * 25))
    thres = np.float32(field.alpha_thres)
    return alpha32 >= thres, np.abs(alpha - float(thres))


def terms(field, params, batches, pde, white_bg=True, app_masks=None, dtype=torch.float64, device="cpu", chunk=256, pde_chunk=32768, kink=0.0):
    """the renders (render64 results, gradients of each MSE) and the PDE term (pde64 result, gradients of the un-weighted L_vel) at `params`.
    batches: [dict(o, d, target, u, t)], the non-keyframe render first; pde: dict(points, t, kept) or None; app_masks: per render a GIVEN (R, S)
    appearance mask or None"""
    load(field, params)
    rs = []
    for k, b in enumerate(batches):
        mask = None if app_masks is None else app_masks[k]
        r = r64.render64(field, b["o"], b["d"], float(b["t"]), b["u"], white_bg, app_mask=mask, loss=r64.Loss(b["target"]), dtype=dtype, device=device,
                         chunk=chunk, acc_dtype=dtype, kink=kink)
        m, _ = optim64.mse(r["rgb"].astype(np.float32), b["target"])
        assert abs(float(m) - r["loss"]) <= 1e-6 * abs(r["loss"]) + 1e-12, ("render64.Loss and optim64.mse disagree", float(m), r["loss"])
        rs.append(r)
    p = None
    if pde is not None:
        ps = pde64.as_params([params[n] for n in pde64.NAMES], device, dtype)
        p = pde64.pde64(pde["points"], pde["t"], pde["kept"], ps, field.aabb.numpy(), grads=True, chunk=pde_chunk, acc_dtype=dtype)
    return dict(renders=rs, pde=p)


def combine(params, m, v, it, T, K, dtype=torch.float64, variant=None, g_prev=None, reg_params=None):
    """the iteration from its terms T: the regularisers at reg_params (default params), the schedule of `it`, the shares, their sum, the Adam step
    of `params` with the moments m, v ({name: fp32 array}; every name of `params` is stepped, with a zero gradient where no term reaches it)"""
    nd = _np(dtype)
    s = schedule(it, variant)
    L1w, tvd, tva, vw = s["w"]
    rp = params if reg_params is None else reg_params
    (L1, TVd, TVa), rg = optim64.regs([rp[n] for n in REG_NAMES], K, (L1w, tvd, tva), dtype=nd)
    shares = dict(r1={}, r2={}, regs={}, pde={})
    rs = T["renders"]
    for key, r in zip(("r1", "r2") if len(rs) == 2 else ("r2",), rs):
        shares[key] = {n: g.astype(nd) for n, g in r["grads"].items() if g is not None}
    shares["regs"] = {n: g.astype(nd) * (nd(2) if variant == "g" else nd(1)) for n, g in zip(REG_NAMES, rg)}
    lv, n_kept = 0.0, 0
    if T["pde"] is not None and T["pde"]["n_kept"] > 0:
        lv, n_kept = T["pde"]["loss"], T["pde"]["n_kept"]
        w = nd(np.float32(vw))                       # the C ABI and the device record carry the weight as fp32
        shares["pde"] = {n: w * g.astype(nd) for n, g in T["pde"]["grads"].items()}
    drop = {"f1": "pde", "f2": "r1"}.get(variant)
    g, p_new, m_new, v_new = {}, {}, {}, {}
    for n in params:
        tot = np.zeros(np.shape(params[n]), nd)
        for key in ("r1", "r2", "regs", "pde"):
            if n in shares[key] and not (key == drop and n.startswith("vel_net.weight_net")):
                tot = tot + shares[key][n].reshape(tot.shape)
        if variant == "d":
            tot = tot + np.asarray(g_prev[n], nd).reshape(tot.shape)
        g[n] = tot
        lr = s["lr_plane"] if "plane" in n else s["lr_net"]
        p_new[n], m_new[n], v_new[n] = optim64.adam(params[n], [tot], [lr], B1, B2, EPS, m0=m[n], v0=v[n], t0=s["t_bias"] - 1, dtype=nd)
    mses = [r["loss"] for r in rs]
    total = float(sum(mses) + L1w * float(L1) + tvd * float(TVd) + tva * float(TVa) + (vw * lv if n_kept else 0.0))
    return dict(rgb=[r["rgb"] for r in rs], mse=mses, regs=(float(L1), float(TVd), float(TVa)), lv=float(lv), n_kept=n_kept, loss=total,
                grads=g, shares=shares, p=p_new, m=m_new, v=v_new, schedule=s, renders=rs)


def step64(field, params, m, v, it, batches, pde, white_bg=True, app_masks=None, dtype=torch.float64, device="cpu", variant=None, g_prev=None,
           stale=None):
    """one iteration.  variant "e" takes the terms from `stale` (the previous iteration's parameters) and applies the step to `params`"""
    src = stale if variant == "e" else params
    T = terms(field, src, batches, pde, white_bg, app_masks, dtype, device)
    return combine(params, m, v, it, T, field.K, dtype, variant, g_prev, reg_params=src)


def round32(d):
    return {k: np.asarray(x, np.float32) for k, x in d.items()}


def free_run(field, params, inputs, dtype=torch.float64, device="cpu", variant=None, white_bg=True, it0=0):
    """step64 on its own output over the iterations `inputs` ([dict(batches, points, t)]; the kept set decided by kept64 at the current parameters),
    from zero moments.  Returns the per-iteration results; each holds `kept_margin`, the smallest |alpha - thres| of its kept decision"""
    p = round32(params)
    m = {k: np.zeros_like(x) for k, x in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    outs, g_prev, p_prev = [], None, None
    for k, inp in enumerate(inputs):
        load(field, p)
        kept, dist = kept64(field, inp["points"], inp["t"], dtype, device)
        pde = dict(points=inp["points"], t=inp["t"], kept=kept)
        var = variant if not (variant in ("d", "e") and k == 0) else None
        o = step64(field, p, m, v, it0 + k, inp["batches"], pde, white_bg, None, dtype, device, var, g_prev, p_prev)
        o["kept_margin"] = float(dist.min())
        outs.append(o)
        g_prev, p_prev = o["grads"], p
        p, m, v = round32(o["p"]), round32(o["m"]), round32(o["v"])
    return outs
