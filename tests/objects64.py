"""Float64 restatement of the object branches of an eval-mode render (include/nvfi_hip.h: nvfi_render_objects, nvfi_render_fwd_select; the reference
has no such calls - their pieces are the reference's own render_pts, models/tensorf_keyframe.py:641-755, and MaskField, models/mask_field.py:68-83
as train_segm.py:97-102 builds it): the yardstick of tests/test_objects_golden.py (against maps composited from the reference's own weights,
renderModule colours and mask_field outputs) and of tests/test_gpu_objects.py (against the device).  Built on render64's pieces (sample_rays,
time_plan, _vel, _planes, _mlp_in); render64._chunk itself has no place to scale the density, so the render is written out again here, eval mode
only, without the loss and the graph cuts.  The contract, restated:

  MaskField(x) = softmax(W4 relu(W3 relu(W2 relu(W1 relu(W0 x + b0) + b1) + b2) + b3) + b4), 3 -> 128 x 4 -> K
  x_j   the warped keyframe position of sample j (where its density and colour are looked up); m_jk = MaskField(x_j)_k
  select given:  s(x) = sum_k select_k m_k(x),  sigma' = sigma s(x) for every valid sample; everything downstream (alpha, transmittance, weights,
        the w > thres appearance mask, colours, composite, depth, acc, background) runs on sigma'.  select None: the plain render.
  M_r   the samples of ray r with weight > float32(rayMarch_weight_thres), decided on a GIVEN fp32 weight map (the device's, or the reference's)
        when one is passed (the way flow64 takes the device's weights), else on the yardstick's own weights
  obj_acc[r][k]   = sum_{j in M_r} w_j m_jk        obj_rgb[r][k] = sum_{j in M_r} w_j m_jk c_j        obj_depth[r][k] = sum_{j in M_r} w_j m_jk z_j
        (c_j the colour the composite uses; premultiplied, no background, no clamp, no (1 - acc) far term); pre_rgb[r] = sum_{j in M_r} w_j c_j

As in render64, what is fixed before the field is touched stays fp32-rounded (rays, sample depths and positions, t, the RK2 schedule, select, the
MaskField parameters' VALUES) and the discrete decisions (box membership, gate, step rejection, appearance mask) are taken on fp32-rounded values;
everything else runs in `dtype`.  dtype=float32 is "a plain fp32 implementation" of the same statement: its distance from the float64 run is the
noise floor the bounds of both test files are derived from.  Samples whose OWN weight lies within 4 fp32 ulp of the threshold are reported
(`near_samples`, `near_rays`): there an fp32 evaluation may decide the appearance mask the other way.  The ulp is that of 1.0 (4 ulp = 4.8e-7),
not of the threshold's own magnitude: w = alpha T with alpha = 1 - exp(-sigma dist), and the subtraction from 1 leaves an ABSOLUTE error of half
an ulp of 1.0 in alpha however small alpha is, so a weight near 1e-4 is uncertain by ulps of 1.0 (times T <= 1), not by ulps of 1e-4 (7e-12)."""
import numpy as np
import torch
import torch.nn.functional as F

import render64 as r64

LAYER_KEYS = ("obj_rgb", "obj_acc", "obj_depth")
MAP_KEYS = ("rgb", "depth", "acc", "weight")
MAP_RTOL = 5e-5          # tests/test_gpu_render64.py: maps within MAP_RTOL x |ref| + helpers.FP32_FLOOR element-wise
MAX_ASIDE = 0.02         # rays that hold a near-threshold sample may be set aside: at most this share of a case's rays

# The plain-fp32 noise floor of the layer sums: max |objects64(float32) - objects64(float64)| / max |objects64(float64)| per map (obj_rgb, obj_acc,
# obj_depth) on the golden cases, both runs on the fixture's weight map.  Measured on the CPU by tests/golden/make_golden_objects.py (which prints
# and records them; tests/test_objects_golden.py measures them again and fails when one exceeds its entry here), rounded up to two digits.
GOLDEN_FLOOR = {
    "A:ko": (3.8e-07, 3.4e-07, 3.6e-07),
    "A:kr": (3.7e-07, 4.0e-07, 3.0e-07),
    "A:no": (6.0e-07, 5.0e-07, 4.6e-07),
    "A:nr": (5.6e-07, 4.6e-07, 5.0e-07),
    "A:ni": (5.0e-07, 4.4e-07, 4.8e-07),
    "A:nf": (6.3e-07, 4.8e-07, 5.3e-07),
    "A:xo": (4.5e-07, 4.6e-07, 4.2e-07),
    "A:xr": (4.7e-07, 4.5e-07, 4.1e-07),
    "B:ko": (1.4e-07, 1.3e-07, 1.5e-07),
    "B:kr": (1.7e-07, 1.4e-07, 1.6e-07),
    "B:no": (1.8e-07, 1.4e-07, 1.3e-07),
    "B:nr": (1.3e-07, 1.4e-07, 1.3e-07),
    "B:ni": (1.6e-07, 1.1e-07, 1.5e-07),
    "B:nf": (1.4e-07, 1.5e-07, 1.3e-07),
    "B:xo": (1.6e-07, 1.1e-07, 1.6e-07),
    "B:xr": (1.7e-07, 1.5e-07, 1.1e-07),
}


def mask_params(sd, prefix=""):
    """[W0, b0, ..., W4, b4] (fp32 numpy) from a MaskField state_dict (point_fc.{0..3}.{weight,bias}, mask_fc.{weight,bias})"""
    names = [f"point_fc.{i}" for i in range(4)] + ["mask_fc"]
    out = []
    for n in names:
        for wb in ("weight", "bias"):
            v = sd[prefix + n + "." + wb]
            out.append(np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32))
    return out


def mask_field(params, x, dtype=torch.float64):
    """softmax mask (n, K) of the points x (n, 3) in `dtype`"""
    h = x.to(dtype)
    for l in range(5):
        h = F.linear(h, torch.as_tensor(params[2 * l]).to(dtype), torch.as_tensor(params[2 * l + 1]).to(dtype))
        if l < 4:
            h = torch.relu(h)
    return torch.softmax(h, -1)


def objects64(field, mparams, rays_o, rays_d, t, white_bg, select=None, transfer=False, weights=None, dtype=torch.float64):
    """One eval-mode render with object selection and layers -> dict (numpy, `dtype`): rgb, depth, acc, weight (the yardstick's own maps under
    `select`), pre_rgb, mask_map (= obj_acc), obj_rgb (R,K,3), obj_acc, obj_depth (on `weights` (R,S) fp32 if given, else on its own weights),
    mask (R,S) the appearance mask the layers used, own_mask, M, near_samples ((n,2) ray, sample), near_rays, s (R,S) the selection factor"""
    smp = r64.sample_rays(field, rays_o, rays_d, None)
    plan = r64.time_plan(field, t, transfer)
    valid = smp["valid"]
    R, S = valid.shape
    P = {k: v.to(dtype) for k, v in field.p32.items()}
    K = int(np.asarray(mparams[8]).shape[0])
    thres = torch.tensor(field.thres, dtype=torch.float32)
    with torch.no_grad():
        xn = smp["xn"].to(dtype)
        z = smp["z"].to(dtype)
        dists = smp["dists"].to(dtype)
        vi = valid.reshape(-1).nonzero()[:, 0]
        x = xn.reshape(-1, 3)[vi]
        for tc, dt, tm in plan["steps"]:
            v1, _ = r64._vel(P, x, tc, field, dtype)
            v2, _ = r64._vel(P, x - 0.5 * dt * v1, tm, field, dtype)
            xc = x - dt * v2
            if field.sur:
                c32 = xc.to(torch.float32)
                out = ((c32 < field.lo) | (c32 > field.hi)).any(-1)
                xc = torch.where(out[:, None], x, xc)
            x = xc
        x4 = torch.cat([x, torch.full_like(x[:, :1], plan["tn_base"])], 1)
        sig_v = F.softplus(r64._planes(P, "density", x4).sum(0) + field.shift)
        s_full = torch.ones(R * S, dtype=dtype)
        if select is not None:
            sel = torch.as_tensor(np.asarray(select, np.float32)).to(dtype)
            s_v = (mask_field(mparams, x, dtype) * sel).sum(-1)
            sig_v = sig_v * s_v
            s_full = s_full.index_put((vi,), s_v)
        sigma = torch.zeros(R * S, dtype=dtype).index_put((vi,), sig_v).view(R, S)
        alpha = 1.0 - torch.exp(-sigma * dists)
        T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dtype), 1.0 - alpha + 1e-10], -1), -1)
        weight = alpha * T[:, :-1]
        own = weight > field.thres
        tol = 4 * float(np.spacing(np.float32(1.0)))
        near = ((weight.to(torch.float64) - float(thres)).abs() <= tol).nonzero().numpy()
        if weights is None:
            mask, w = own, weight
        else:
            w32 = torch.as_tensor(np.asarray(weights, np.float32)).reshape(R, S)
            mask, w = w32 > thres, w32.to(dtype)
        # colours of the own mask (the render's maps) and of the layer mask: one evaluation over their union
        both = (own | mask).reshape(-1)
        mi = both.nonzero()[:, 0]
        rgb_s = torch.zeros(R * S, 3, dtype=dtype)
        m_s = torch.zeros(R * S, K, dtype=dtype)
        if mi.numel():
            pos = torch.full((R * S,), -1, dtype=torch.long).index_put((vi,), torch.arange(vi.numel()))
            pm = pos[mi]
            raw = torch.cat([xn.reshape(-1, 3)[mi], torch.full_like(xn.reshape(-1, 3)[mi][:, :1], plan["tn_base"])], 1)
            x4m = torch.where((pm >= 0)[:, None], x4[pm.clamp(min=0)], raw)       # (a masked sample is a valid one; an invalid one reads the raw point)
            view = smp["d"].to(dtype)[:, None, :].expand(R, S, 3).reshape(-1, 3)[mi]
            h = r64._mlp_in(P, x4m, view)
            for i in (0, 2, 4):
                h = F.linear(h, P[f"renderModule.mlp.{i}.weight"], P[f"renderModule.mlp.{i}.bias"])
                h = torch.relu(h) if i < 4 else torch.sigmoid(h)
            rgb_s = rgb_s.index_put((mi,), h)
            m_s = m_s.index_put((mi,), mask_field(mparams, x4m[:, :3], dtype))
        rgb_s, m_s = rgb_s.view(R, S, 3), m_s.view(R, S, K)
        wo = weight * own
        acc = weight.sum(-1)
        rgb_map = (wo[..., None] * rgb_s).sum(-2)
        if white_bg:
            rgb_map = rgb_map + (1.0 - acc[..., None])
        depth = (weight * z).sum(-1) + (1.0 - acc) * field.far
        wl = w * mask
        wm = wl[..., None] * m_s                                   # (R, S, K)
        res = dict(rgb=rgb_map.clamp(0, 1), depth=depth, acc=acc, weight=weight, pre_rgb=(wl[..., None] * rgb_s).sum(-2),
                   obj_acc=wm.sum(1), obj_rgb=(wm[..., None] * rgb_s[:, :, None, :]).sum(1), obj_depth=(wm * z[..., None]).sum(1),
                   s=s_full.view(R, S))
    out = {k: v.numpy() for k, v in res.items()}
    out["mask_map"] = out["obj_acc"]
    out["mask"], out["own_mask"], out["M"] = mask.numpy(), own.numpy(), int(mask.sum())
    out["valid"] = valid.numpy()
    out["near_samples"] = near
    out["near_rays"] = np.unique(near[:, 0]) if len(near) else np.zeros(0, np.int64)
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 for an all-zero reference that is matched exactly)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    return 0.0 if err == 0.0 else float(err / scale) if scale > 0 else float("inf")


def ulp_floor(ref):
    """one fp32 ulp of the map's scale, relative to it: no fp32 map is better than its last bit"""
    scale = float(np.abs(np.asarray(ref, np.float64)).max()) if np.asarray(ref).size else 0.0
    return float(np.spacing(np.float32(scale))) / scale if scale > 0 else 0.0


def layer_floor(y32, y64):
    """per LAYER_KEYS: the plain-fp32 floor of a case, never below one ulp of the map scale"""
    return tuple(max(rel_err(y32[k], y64[k]), ulp_floor(y64[k])) for k in LAYER_KEYS)


def map_failures(got, ref, floors):
    """{key: ray indices} where a map of a selected render leaves MAP_RTOL x |ref| + floors[key] element-wise (tests/test_gpu_render64.py's rule)"""
    bad = {}
    for k in MAP_KEYS:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        ok = np.abs(g - r) <= MAP_RTOL * np.abs(r) + floors[k]
        rows = np.nonzero(~ok.reshape(ok.shape[0], -1).all(1))[0]
        if len(rows):
            bad[k] = rows
    return bad
