"""Float64 restatement, with autograd, of one render of the reference's TensorVMKeyframeTimeKplane (models/tensorf_keyframe.py:613-755, forward /
render_pts) and of the loss on its maps: the yardstick of tests/test_render64_golden.py (against the reference's goldens) and of
tests/test_gpu_render64.py (against the device kernels).  Written out from the mathematics:

  sample_ray (tensorf_base.py:290-314) with a GIVEN per-ray jitter u: z_j = t_min + stepSize (j + u), p = o + d z, valid = p inside the box;
      t_min = near if ANY origin coordinate of the batch lies in its box range, else the slab entry clamped to [near, far].
  normalize_coord (tensorf_base.py:241): (p - aabb0) * (2 / size) - 1;  normalize_time_coord (tensorf_keyframe.py:501-506): 2 t / tmax - 1.
  base keyframe time (tensorf_keyframe.py:646-654): round(clamp(t / dt_k, 0, K - 1)) dt_k with dt_k = tmax / (K - 1); 0 with transfer_vel.
  integrate_pos (tensorf_keyframe.py:575-611): RK2 steps of |dt| <= dt_k / 2 from t back to the base time through the gated velocity net,
      x <- x - dt v(x - dt/2 v(x, t), t - dt/2); VelocityAABB (velocity_field.py:21-33) gates v to 0 outside [-1 + eps, 1 - eps]^3,
      VelocityAABBSur (velocity_field.py:36-51) outside the normalised surround box, and with it a step that leaves that box is rejected
      (tensorf_keyframe.py:602-604).  A time with isclose(t, base) is a keyframe: no warp (tensorf_keyframe.py:684-693).  The
      `base_times == tmax` out-of-range rule (tensorf_keyframe.py:701-703) rewrites xyzt_sampled, which nothing reads afterwards: every lookup
      below uses the warped point and the base time, in range or not.
  compute_densityfeature (tensorf_keyframe.py:233-272): sum over channels of prod_i space_i(x_a, x_b) time_i(x_c, t), bilinear
      F.grid_sample(align_corners=True, zero padding), plane i over the axes (0,1), (0,2), (1,2) and its time plane over (2,t), (1,t), (0,t).
  feature2density (tensorf_keyframe.py:312-326): softplus(feature + density_shift).
  raw2alpha (tensorf_model_utils.py:186-197): alpha = 1 - exp(-sigma dist distance_scale), T = cumprod(1 - alpha + 1e-10), w = alpha T.
  appearance mask w > rayMarch_weight_thres; compute_appfeature (tensorf_keyframe.py:274-310) the same product with the appearance planes, then
      basis_mat; MLPRender_PE (tensorf_base.py:67-98): sigmoid(MLP([feat, view, x, PE6(x), PE6(view)])), PE = [sin(2^k q), cos(2^k q)], ReLU.
  composite (tensorf_keyframe.py:735-746): acc = sum w, rgb = sum w c (+ 1 - acc on white), clamp(0, 1), depth = sum w z + (1 - acc) far.

What the reference produces in fp32 BEFORE the field is touched stays fp32-rounded and is then promoted: ray origins / directions, the jitter, the
sample depths and positions, the sample distances, the normalised coordinates, the time, the base time, the RK2 step schedule (a per-call scalar
recurrence) and their normalised forms.  Everything after that runs in `dtype` (float64; float32 gives "a plain fp32 implementation" of the same
statement, the noise floor the bounds are derived from).  The discrete decisions are taken on fp32-rounded values like the reference's: box
membership on the fp32 positions, the velocity gate and step rejection on the fp32 rounding of the current point, the appearance mask on the
weight in `dtype` against float32(thres) - or GIVEN (`app_mask`: the device's own, read off its weight map), in which case the samples where the
given mask and the yardstick's differ are reported with their |w - thres|.

Rays are independent: they are processed in chunks, and the gradients accumulate over the chunks in float64 (acc_dtype: in another dtype).  The loss has to be a sum over rays:
a `Loss` (mse + w_depth mean(depth) + w_acc mean(acc^2) + sum(weight gw): the golden loss; w_depth = w_acc = 0 and no gw is the bench's mse) or a
callable (rgb, depth, acc, weight, ray_index, R) -> per-ray terms.

Eval-time culling (tensorf_keyframe.py:656-661; AlphaGridMask.sample_alpha, tensorf_model_utils.py:433-439) is restated through `alpha_volume`:
in an eval call (jitter None) an in-box sample stays valid only where the trilinear read of the (D, H, W) occupancy volume is > 0.  The volume is
read at the FIELD's normalised coordinates - sample_alpha's own normalize_coord is commented out in the reference - so a mask that was built before
shrink() is read in the new box's coordinates (tests/alpha64.py: sample_alpha64 holds the lookup and says which samples sit on a voxel boundary).

shadingMode "SH" (tensorf_base.py:196-197; SHRender, tensorf_model_utils.py:292-296, sh.py:87-110): app_dim = 27, basis_mat is 48 -> 27 and the
colour of a masked sample is relu(sum_k SH_k(view) feat[9 c + k] + 0.5) with the degree-2 real basis on the RAW view direction (_sh_basis) - no
positional encoding, no MLP, no sigmoid: the colour is unbounded above, so the clamp(0, 1) of the composite is live in this mode.  Such a field
(`Field.sh`) has no renderModule.* parameter: `Field.names` leaves the six out.  `wrong=True` is the one deliberately wrong variant of this file
(SH fields only): basis 6 formed with zz - xx - yy instead of 2 zz - xx - yy; both test files show that their bounds see it.

Parameters are keyed by the reference's names without the `nvfi.` prefix, as helpers.named_grads gives them."""
import numpy as np
import torch
import torch.nn.functional as F

import pde64

MAT_SPACE = [(0, 1), (0, 2), (1, 2)]
MAT_TIME = [(2, 3), (1, 3), (0, 3)]
VEL_NAMES = pde64.NAMES[:12]
PLANE_NAMES = [f"{b}_plane_{st}.{i}" for b in ("density", "app") for st in ("space", "time") for i in range(3)]
MLP_NAMES = [f"renderModule.mlp.{i}.{wb}" for i in (0, 2, 4) for wb in ("weight", "bias")]
NAMES = PLANE_NAMES + ["basis_mat.weight"] + MLP_NAMES + VEL_NAMES
SH_NAMES = [n for n in NAMES if n not in MLP_NAMES]          # an SH field: basis_mat.weight stays in family `mlp`
FAMILY = {n: ("density" if n.startswith("density") else "app" if n.startswith("app") else "vel" if n.startswith("vel_net") else "mlp") for n in NAMES}


class Field:
    """the parameters (fp32 values, reference layout) and the configuration scalars that reach the render"""

    def __init__(self, sd, meta, sh=None):
        sd = {(k[5:] if k.startswith("nvfi.") else k): np.asarray(v) for k, v in sd.items()}
        # SH shading: said by the caller, or read off the parameters (basis_mat 48 -> 27 and no render MLP)
        self.sh = (tuple(sd["basis_mat.weight"].shape) == (27, 48) and not any(k.startswith("renderModule.") for k in sd)) if sh is None else bool(sh)
        self.p32 = {k: torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)) for k in NAMES if not (self.sh and k in MLP_NAMES and k not in sd)}
        m = meta
        self.aabb = torch.from_numpy(np.asarray(m["aabb"], np.float32).reshape(2, 3).copy())
        self.near, self.far = float(m["near"]), float(m["far"])
        self.step, self.S = float(m["stepSize"]), int(m["nSamples"])
        self.K, self.tmax = int(m["num_keyframes"]), float(m["tmax"])
        self.shift, self.dscale = float(m["density_shift"]), float(m["distance_scale"])
        self.thres = float(np.float32(float(m["rayMarch_weight_thres"])))      # an fp32 tensor against a Python scalar compares in fp32
        self.sur = bool(int(m.get("use_sur", 0)))
        if self.sur:
            b = np.asarray(m["sur_bounds"], np.float32).reshape(2, 3)
            self.lo, self.hi = torch.from_numpy(b[0].copy()), torch.from_numpy(b[1].copy())
        else:
            eps = float(m.get("eps", 0.03))
            self.lo = torch.full((3,), float(np.float32(-1 + eps)), dtype=torch.float32)
            self.hi = torch.full((3,), float(np.float32(1 - eps)), dtype=torch.float32)

    @property
    def names(self):
        """the parameters a render of this field can reach (NAMES; without the render MLP's on an SH field)"""
        return SH_NAMES if self.sh else NAMES


class Loss:
    """mse(rgb, target) + w_depth mean(depth) + w_acc mean(acc^2) + sum(weight * gw), as per-ray terms"""

    def __init__(self, target, w_depth=0.0, w_acc=0.0, gw=None, keep=None):
        """keep (R, 3) bool: the channels whose mse term is kept (default: all) - what a test cuts to show that a channel carries no gradient"""
        self.keep = None if keep is None else torch.as_tensor(np.asarray(keep, bool)).reshape(-1, 3)
        self.target = torch.as_tensor(np.asarray(target, np.float32)).reshape(-1, 3)
        self.w_depth, self.w_acc = float(w_depth), float(w_acc)
        self.gw = None if gw is None else torch.as_tensor(np.asarray(gw, np.float32))

    def __call__(self, rgb, depth, acc, weight, idx, R):
        tg = self.target[idx].to(rgb)
        sq = (rgb - tg) ** 2
        out = (sq if self.keep is None else sq * self.keep[idx].to(rgb)).sum(-1) / (3 * R)
        if self.w_depth:
            out = out + self.w_depth * depth / R
        if self.w_acc:
            out = out + self.w_acc * acc * acc / R
        if self.gw is not None:
            out = out + (weight * self.gw[idx].to(rgb)).sum(-1)
        return out


# ---------------------------------------------------------------------------------------------------------------- fp32 inputs
def sample_rays(field, rays_o, rays_d, jitter):
    """sample_ray + normalize_coord in fp32 (CPU): positions are not kept, only what the render reads.  jitter None: eval mode (no jitter)"""
    o = torch.as_tensor(np.asarray(rays_o, np.float32)).reshape(-1, 3)
    d = torch.as_tensor(np.asarray(rays_d, np.float32)).reshape(-1, 3)
    a0, a1 = field.aabb[0], field.aabb[1]
    if ((a0 <= o) & (o <= a1)).any():
        t_min = torch.ones_like(o[..., 0]) * field.near
    else:
        vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
        t_min = torch.minimum((a1 - o) / vec, (a0 - o) / vec).amax(-1).clamp(min=field.near, max=field.far)
    rng = torch.arange(field.S)[None].float()
    if jitter is not None:
        rng = rng.repeat(o.shape[0], 1)
        rng += torch.as_tensor(np.asarray(jitter, np.float32)).reshape(-1, 1)
    z = t_min[..., None] + field.step * rng
    pts = o[..., None, :] + d[..., None, :] * z[..., None]
    valid = ~((a0 > pts) | (pts > a1)).any(-1)
    dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), -1) * field.dscale
    inv = 2.0 / (a1 - a0)
    xn = (pts - a0) * inv - 1
    return dict(o=o, d=d, z=z, valid=valid, dists=dists, xn=xn)


def time_plan(field, t, transfer=False):
    """the base time, the keyframe decision and the RK2 schedule [(t_curr, dt), ...] of one call, computed in fp32 like the reference's tensors"""
    t32 = torch.tensor(float(t), dtype=torch.float32)
    if not getattr(field, "use_vel", True):
        # a radiance-only field (use_vel False, tensorf_keyframe.py:703-704): no warp, every lookup at the CONTINUOUS normalised frame time
        tn = t32 * 0 if field.tmax == 0 else t32 * 2 / field.tmax - 1
        return dict(base=float(t32), key=True, steps=[], tn_base=float(tn))
    scale = field.tmax / (field.K - 1) if field.K > 1 else 1
    base = torch.zeros_like(t32) if transfer else torch.round((t32 / scale).clamp(0.0, field.K - 1)) * scale
    key = bool(torch.isclose(t32, base))
    steps = []
    if not key:
        dt_max = torch.ones_like(t32) * (0.5 * field.tmax / (field.K - 1) if field.K > 1 else 1)
        off, cur = t32 - base, t32.clone()
        while bool(off.abs() > 0):
            dt = off.sign() * torch.minimum(off.abs(), dt_max)
            steps.append((float(cur), float(dt), float(cur - 0.5 * dt)))
            off, cur = off - dt, cur - dt
    tn = base * 0 if (field.K == 1 or field.tmax == 0) else base * 2 / field.tmax - 1
    return dict(base=float(base), key=key, steps=steps, tn_base=float(tn))


# ---------------------------------------------------------------------------------------------------------------- the field in `dtype`
def _planes(P, which, x4):
    """(C, n): prod over the three plane pairs of space_i * time_i at the points x4 (n, 4) = (x, y, z, normalised time)"""
    out = None
    for i in range(3):
        gs = x4[:, list(MAT_SPACE[i])].view(1, -1, 1, 2)
        gt = x4[:, list(MAT_TIME[i])].view(1, -1, 1, 2)
        ps, pt = P[f"{which}_plane_space.{i}"], P[f"{which}_plane_time.{i}"]
        a = F.grid_sample(ps, gs, align_corners=True).view(ps.shape[1], x4.shape[0])          # (the channel count is spelt out: n may be 0)
        b = F.grid_sample(pt, gt, align_corners=True).view(pt.shape[1], x4.shape[0])
        out = a * b if out is None else out * (a * b)
    return out


def _vel(P, x, tt, field, dtype):
    """gated velocity at the points x (n, 3) and the scalar time tt; returns v and the in-gate mask"""
    x32 = x.detach().to(torch.float32)
    inside = ~((x32 < field.lo.to(x.device)) | (x32 > field.hi.to(x.device))).any(-1)
    v = torch.zeros_like(x)
    if inside.any():
        xi = x[inside]
        q = torch.cat([xi, torch.full_like(xi[:, :1], tt)], 1)
        w = pde64._mlp(q, [P[n] for n in VEL_NAMES[0::2]], [P[n] for n in VEL_NAMES[1::2]], F.silu)
        px, py, pz = xi[:, 0], xi[:, 1], xi[:, 2]
        vi = torch.stack([w[:, 0] - w[:, 4] * pz + w[:, 5] * py, w[:, 1] + w[:, 3] * pz - w[:, 5] * px, w[:, 2] - w[:, 3] * py + w[:, 4] * px], 1)
        v = v.index_put((inside.nonzero()[:, 0],), vi)
    return v, inside


def _pe(q, n):
    f = (q[..., None] * (2.0 ** torch.arange(n, dtype=q.dtype, device=q.device))).reshape(q.shape[:-1] + (n * q.shape[-1],))
    return torch.cat([torch.sin(f), torch.cos(f)], -1)


def _sh_basis(view, wrong=False):
    """(n, 9): the real spherical harmonics of degree <= 2 at the raw (un-normalised) view direction, in sh.py's order and signs"""
    C0, C1 = 0.28209479177387814, 0.4886025119029199
    C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    x, y, z = view[:, 0], view[:, 1], view[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b6 = (zz - xx - yy) if wrong else (2.0 * zz - xx - yy)
    return torch.stack([torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x, C2[0] * xy, C2[1] * yz, C2[2] * b6, C2[3] * xz, C2[4] * (xx - yy)], 1)


def _sh_pre(view, feat27, wrong=False):
    """(n, 3, 9) terms SH_k(view) feat[9 c + k] and (n, 3) their sum + 0.5, the colour before its ReLU"""
    terms = _sh_basis(view, wrong)[:, None, :] * feat27.view(-1, 3, 9)
    return terms, terms.sum(-1) + 0.5


def _sh(view, feat27, wrong):
    """SHRender: relu(sum_k SH_k(view) feat[9 c + k] + 0.5), (n, 3).  wrong: basis 6 with zz - xx - yy instead of 2 zz - xx - yy"""
    return torch.relu(_sh_pre(view, feat27, wrong)[1])


def _mlp_in(P, x4m, view):
    feat = F.linear(_planes(P, "app", x4m).T, P["basis_mat.weight"])
    xm = x4m[:, :3]
    return torch.cat([feat, view, xm, _pe(xm, 6), _pe(view, 6)], -1)


def _chunk(field, P, smp, sl, plan, white_bg, app_mask, loss, R, dtype, device, cut_rgb=None, cut_sigma=None, want_margin=False, cut_warp=None,
           wrong=False, kink=0.0):
    """one chunk of rays sl (index array): the maps, the masks, the per-ray loss terms (a tensor still attached to the graph)"""
    idx = torch.as_tensor(sl, dtype=torch.long)
    valid = smp["valid"][idx].to(device)
    r, S = valid.shape
    xn = smp["xn"][idx].to(device=device, dtype=dtype)
    z = smp["z"][idx].to(device=device, dtype=dtype)
    dists = smp["dists"][idx].to(device=device, dtype=dtype)
    view = smp["d"][idx].to(device=device, dtype=dtype)
    vi = valid.reshape(-1).nonzero()[:, 0]
    x = xn.reshape(-1, 3)[vi]
    in_gate = torch.zeros(r * S, dtype=torch.bool, device=device)
    for k, (tc, dt, tm) in enumerate(plan["steps"]):
        v1, ins = _vel(P, x, tc, field, dtype)
        if k == 0:
            in_gate[vi] = ins
        v2, _ = _vel(P, x - 0.5 * dt * v1, tm, field, dtype)
        xc = x - dt * v2
        if field.sur:
            c32 = xc.detach().to(torch.float32)
            out = ((c32 < field.lo.to(device)) | (c32 > field.hi.to(device))).any(-1)
            xc = torch.where(out[:, None], x, xc)
        x = xc
    if cut_warp is not None and plan["steps"]:
        x = torch.where(cut_warp[idx].to(device).reshape(-1)[vi][:, None], x.detach(), x)
    x4 = torch.cat([x, torch.full_like(x[:, :1], plan["tn_base"])], 1)
    sig_v = F.softplus(_planes(P, "density", x4).sum(0) + field.shift)
    if cut_sigma is not None:
        cs = cut_sigma[idx].to(device).reshape(-1)[vi]
        sig_v = torch.where(cs, sig_v.detach(), sig_v)
    sigma = torch.zeros(r * S, dtype=dtype, device=device).index_put((vi,), sig_v).view(r, S)
    alpha = 1.0 - torch.exp(-sigma * dists)
    T = torch.cumprod(torch.cat([torch.ones(r, 1, dtype=dtype, device=device), 1.0 - alpha + 1e-10], -1), -1)
    weight = alpha * T[:, :-1]
    own = weight.detach() > field.thres
    mask = own if app_mask is None else torch.as_tensor(app_mask[sl], dtype=torch.bool).to(device)
    rgb = torch.zeros(r * S, 3, dtype=dtype, device=device)
    margin = None
    mi = mask.reshape(-1).nonzero()[:, 0]
    if mi.numel():
        # a masked sample is a valid one unless the GIVEN mask says otherwise: look the point up in the valid list (invalid ones read the raw point)
        pos = torch.full((r * S,), -1, dtype=torch.long, device=device).index_put((vi,), torch.arange(vi.numel(), device=device))
        pm = pos[mi]
        x4m = torch.where((pm >= 0)[:, None], x4[pm.clamp(min=0)],
                          torch.cat([xn.reshape(-1, 3)[mi], torch.full_like(xn.reshape(-1, 3)[mi][:, :1], plan["tn_base"])], 1))
        vm = view[:, None, :].expand(r, S, 3).reshape(-1, 3)[mi]
        if field.sh:
            terms_sh, pre = _sh_pre(vm, F.linear(_planes(P, "app", x4m).T, P["basis_mat.weight"]), wrong)
            if want_margin:       # |pre| over the fp32 rounding bound of its ten-term sum (nine products and the 0.5), per channel
                margin = (pre.abs() / ((terms_sh.abs().sum(-1) + 0.5) * (2.0 ** -24 * 10))).detach()
            h = torch.relu(pre)
        else:
            h = _mlp_in(P, x4m, vm)
            if want_margin:
                margin = torch.full((mi.numel(),), float("inf"), dtype=dtype, device=device)
        for i in () if field.sh else (0, 2, 4):
            W, b = P[f"renderModule.mlp.{i}.weight"], P[f"renderModule.mlp.{i}.bias"]
            zz = F.linear(h, W, b)
            if (want_margin or kink) and i < 4:
                err = (F.linear(h.abs(), W.abs()) + b.abs()) * (2.0 ** -24 * h.shape[1])
            if want_margin and i < 4:
                margin = torch.minimum(margin, (zz.abs() / err).min(1).values).detach()
            if kink and i < 4:       # the ReLU DECISION taken `kink` rounding bounds beside the pre-activation (the value passed on is still zz)
                h = torch.where((zz + kink * err).detach() > 0, zz, torch.zeros_like(zz))
            else:
                h = torch.relu(zz) if i < 4 else torch.sigmoid(zz)
        if cut_rgb is not None:
            cr = cut_rgb[idx].to(device).reshape(-1)[mi]
            h = torch.where(cr[:, None], h.detach(), h)
        rgb = rgb.index_put((mi,), h)
    rgb = rgb.view(r, S, 3)
    acc = weight.sum(-1)
    rgb_map = (weight[..., None] * rgb).sum(-2)
    if white_bg:
        rgb_map = rgb_map + (1.0 - acc[..., None])
    rgb_pre = rgb_map
    rgb_map = rgb_map.clamp(0, 1)
    depth = (weight * z).sum(-1) + (1.0 - acc) * field.far
    terms = loss(rgb_map, depth, acc, weight, idx, R) if loss is not None else None
    res = dict(rgb=rgb_map, depth=depth, acc=acc, weight=weight, app_mask=mask, own_mask=own, valid=valid, in_gate=in_gate.view(r, S))
    if margin is not None:
        mg = torch.full((r * S,) + tuple(margin.shape[1:]), float("inf"), dtype=dtype, device=device)
        mg[mi] = margin
        res["margin"] = mg.view((r, S) + tuple(margin.shape[1:]))
    if want_margin and field.sh:
        # the distance of the composited colour from the two kinks of clamp(0, 1) over the fp32 rounding bound of the composite: S products w c
        # and the background term.  A channel that sits EXACTLY on a kink because nothing was added to it (a ray without weight: 0 on black, 1 on
        # white) has no decision to take - every colour gradient of it is multiplied by a zero weight - and is left at inf.
        comp = ((weight[..., None] * rgb).abs().sum(-2) + ((1.0 - acc[..., None]).abs() if white_bg else 0.0)) * (2.0 ** -24 * (S + 1))
        dist = torch.minimum(rgb_pre.abs(), (rgb_pre - 1.0).abs())
        mr = torch.where((dist == 0) & (acc[..., None] == 0), torch.full_like(dist, float("inf")), dist / comp.clamp(min=1e-300))
        res["margin_ray"] = mr.detach()
        res["dead"] = (mask[..., None] & (rgb.detach() == 0)) if mi.numel() else torch.zeros(r, S, 3, dtype=torch.bool, device=device)
    return res, terms


MAP_KEYS = ("rgb", "depth", "acc", "weight", "app_mask", "own_mask", "valid", "in_gate")


def render64(field, rays_o, rays_d, t, jitter, white_bg, app_mask=None, loss=None, transfer=False, grads=True, rays=None, chunk=256,
             dtype=torch.float64, device="cpu", cut_rgb=None, cut_sigma=None, want_margin=False, cut_warp=None, alpha_volume=None, cull_flip=None,
             wrong=False, acc_dtype=torch.float64, kink=0.0):
    """the render of the rays `rays` (default: all; the sampling and the loss's 1 / R always refer to the full batch) -> dict of the maps (numpy),
    `loss_rays` (per-ray loss terms, float64), `loss` (their sum), `grads` {name: float64 array, or None where the parameter is not reached},
    `flips` (indices (ray, sample) where the given app_mask differs from the yardstick's own) and `flip_dist` (their |w - thres|).
    alpha_volume (D, H, W), eval calls only: the in-box samples whose occupancy read is not > 0 are culled; the result then holds `in_box` (R, S; the
    valid map before culling), `culled`, `alpha_near` (in-box samples whose decision may fall the other way, alpha64.sample_alpha64) over ALL rays of
    the batch; cull_flip: (n, 2) (ray, sample) whose culling decision is inverted (what a wrong lookup would do to them)
    acc_dtype: the dtype in which the gradients of the chunks are added up (default float64; a float32 run that is to be a PLAIN fp32 implementation
    down to its sum over the rays passes float32: one rounding per chunk, in chunk order)
    kink (MLP shading): every hidden unit of the render MLP decides its ReLU at z + kink x (the fp32 rounding bound of z, as relu_margin forms it)
    instead of at z.  The results at kink = +1 and -1 bracket what an fp32 evaluation may do at units within rounding of their kink, where the
    parameter gradient jumps: their distance is the width of that ambiguity for the case"""
    smp = sample_rays(field, rays_o, rays_d, jitter)
    R = smp["o"].shape[0]
    cull = None
    if alpha_volume is not None and jitter is None:
        import alpha64
        box = smp["valid"].clone()
        bi = box.reshape(-1).nonzero()[:, 0]
        a, _, nr = alpha64.sample_alpha64(alpha_volume, smp["xn"].reshape(-1, 3)[bi], dtype)
        keep = torch.zeros(box.numel(), dtype=torch.bool).index_put((bi,), torch.from_numpy(a > 0))
        near = torch.zeros(box.numel(), dtype=torch.bool).index_put((bi,), torch.from_numpy(nr))
        keep = keep.view(box.shape)
        if cull_flip is not None:
            for i, j in np.asarray(cull_flip).reshape(-1, 2):
                assert bool(box[i, j]), "only an in-box sample has a culling decision"
                keep[i, j] = ~keep[i, j]
        smp["valid"] = box & keep
        cull = dict(in_box=box.numpy(), culled=(box & ~keep).numpy(), alpha_near=near.view(box.shape).numpy())
    plan = time_plan(field, t, transfer)
    rays = np.arange(R) if rays is None else np.asarray(rays, np.int64)
    P = {k: v.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(grads and loss is not None) for k, v in field.p32.items()}
    assert not wrong or field.sh, "the wrong variant is the SH basis's"
    names = [n for n in field.names if not (n.startswith("vel_net") and not plan["steps"])]
    g = {n: torch.zeros(P[n].shape, dtype=acc_dtype, device=device) for n in names}
    outs = {k: [] for k in MAP_KEYS + ("loss_rays",) + (("margin",) if want_margin else ()) + (("margin_ray", "dead") if want_margin and field.sh else ())}
    for s in range(0, len(rays), chunk):
        sl = rays[s:s + chunk]
        with torch.set_grad_enabled(grads and loss is not None):
            res, terms = _chunk(field, P, smp, sl, plan, white_bg, app_mask, loss, R, dtype, device, cut_rgb, cut_sigma, want_margin, cut_warp, wrong,
                                kink)
            if terms is not None and grads:
                gi = torch.autograd.grad(terms.sum(), [P[n] for n in names], allow_unused=True)
                for n, x in zip(names, gi):
                    if x is not None:
                        g[n] += x.to(acc_dtype)
        for k in outs:
            if k == "loss_rays":
                outs[k].append(np.zeros(len(sl)) if terms is None else terms.detach().to(torch.float64).cpu().numpy())
            else:
                outs[k].append(res[k].detach().cpu().numpy())
    out = {k: np.concatenate(v) for k, v in outs.items()}
    out["rays"], out["R"], out["plan"] = rays, R, plan
    if cull is not None:
        out.update(cull)
    out["loss"] = float(out["loss_rays"].sum())
    out["grads"] = {n: (g[n].to(torch.float64).cpu().numpy() if n in g else None) for n in field.names} if (grads and loss is not None) else None
    diff = out["app_mask"] != out["own_mask"]
    out["flips"] = np.argwhere(diff)
    out["flip_dist"] = np.abs(out["weight"][diff].astype(np.float64) - field.thres)
    out["call"] = dict(field=field, rays_o=rays_o, rays_d=rays_d, t=t, jitter=jitter, white_bg=white_bg, loss=loss, transfer=transfer, chunk=chunk,
                       dtype=dtype, device=device, alpha_volume=alpha_volume, cull_flip=cull_flip, wrong=wrong)
    return out


def with_mask(ref, app_mask):
    """the reference `ref` (a render64 result over its rays) under another appearance mask (R, S): only the rays whose mask rows differ are
    recomputed; their old contribution to the gradient sum is subtracted and the new one added.  Returns a new result."""
    rays = ref["rays"]
    rows = np.nonzero((np.asarray(app_mask, bool)[rays] != ref["app_mask"]).any(1))[0]
    if rows.size == 0:
        return ref
    c = ref["call"]
    full_old = np.zeros((ref["R"], ref["app_mask"].shape[1]), bool)
    full_old[rays] = ref["app_mask"]
    kw = dict(loss=c["loss"], transfer=c["transfer"], chunk=c["chunk"], dtype=c["dtype"], device=c["device"], rays=rays[rows],
              alpha_volume=c["alpha_volume"], cull_flip=c["cull_flip"], wrong=c["wrong"])
    old = render64(c["field"], c["rays_o"], c["rays_d"], c["t"], c["jitter"], c["white_bg"], app_mask=full_old, **kw)
    new = render64(c["field"], c["rays_o"], c["rays_d"], c["t"], c["jitter"], c["white_bg"], app_mask=np.asarray(app_mask, bool), **kw)
    out = dict(ref)
    for k in MAP_KEYS + ("loss_rays",):
        a = ref[k].copy()
        a[rows] = new[k]
        out[k] = a
    out["loss"] = float(out["loss_rays"].sum())
    if ref["grads"] is not None:
        out["grads"] = {n: (None if v is None else v - old["grads"][n] + new["grads"][n]) for n, v in ref["grads"].items()}
    diff = out["app_mask"] != out["own_mask"]
    out["flips"] = np.argwhere(diff)
    out["flip_dist"] = np.abs(out["weight"][diff].astype(np.float64) - c["field"].thres)
    return out


def detach(ref, samples, branch):
    """the gradients of the reference `ref` with one branch of the samples `samples` ((n, 2) array of (row of ref["rays"], sample)) cut out of
    the graph: "rgb" the appearance branch (the sample's colour), "sigma" the density branch, "warp" the back-warp (the RK2 adjoint into the
    velocity net).  full - detach(...) is exactly what a kernel loses when it skips those samples in that part of the backward.  Only the rays
    that hold such samples are recomputed."""
    samples = np.asarray(samples).reshape(-1, 2)
    rows = np.unique(samples[:, 0])
    c = ref["call"]
    rays = ref["rays"]
    S = ref["app_mask"].shape[1]
    cut = torch.zeros(ref["R"], S, dtype=torch.bool)
    cut[torch.as_tensor(rays[samples[:, 0]]), torch.as_tensor(samples[:, 1])] = True
    mask = np.zeros((ref["R"], S), bool)
    mask[rays] = ref["app_mask"]
    kw = dict(app_mask=mask, loss=c["loss"], transfer=c["transfer"], chunk=c["chunk"], dtype=c["dtype"], device=c["device"], rays=rays[rows],
              alpha_volume=c["alpha_volume"], cull_flip=c["cull_flip"], wrong=c["wrong"])
    a = render64(c["field"], c["rays_o"], c["rays_d"], c["t"], c["jitter"], c["white_bg"], **kw)
    b = render64(c["field"], c["rays_o"], c["rays_d"], c["t"], c["jitter"], c["white_bg"], **kw, **{"cut_" + branch: cut})
    return {n: (None if v is None else v - a["grads"][n] + b["grads"][n]) for n, v in ref["grads"].items()}


def relu_margin(field, rays_o, rays_d, t, jitter, app_mask=None, chunk=256, device="cpu", white_bg=True):
    """(R, S): per appearance-masked sample the smallest |z| / (fp32 rounding bound of z) over the 256 hidden units of the render MLP, inf elsewhere.
    Below ~1 an fp32 evaluation may take the other side of a ReLU kink than float64, and the sample's parameter gradient jumps there.
    An SH field has two kinds of kink and returns a pair: (R, S, 3), per masked sample and channel |pre| / (2^-24 x 10 x (sum_k |SH_k feat_k| + 0.5)),
    pre the colour before its ReLU; and (R, 3), per ray and channel, the distance of the composited colour before clamp(0, 1) from 0 and from 1
    over 2^-24 x (S + 1) x (sum_s |w c| + |1 - acc|) (inf for a ray without any weight, which sits on its background exactly).  The render64
    result of an SH field with want_margin also holds `dead` (R, S, 3): the masked (sample, channel) colours that are exactly 0."""
    r = render64(field, rays_o, rays_d, t, jitter, white_bg, app_mask=app_mask, loss=None, grads=False, chunk=chunk, device=device, want_margin=True)
    return (r["margin"], r["margin_ray"]) if field.sh else r["margin"]


def list_order(mask):
    """(n, 2) indices of a compacted list in the device's order: ray-major, sample-minor (render_rays.hip: k_weights_fill / k_fill write per-ray
    offsets from an exclusive scan over the rays, samples in order within a ray)"""
    return np.argwhere(mask)
