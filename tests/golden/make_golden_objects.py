#!/usr/bin/env python
"""Golden vectors of the object branches (nvfi_render_objects, nvfi_render_fwd_select), generated from the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_objects.py        (NVFI_REFERENCE: checkout of the reference; default as in make_golden.py)
The reference has no call that renders these maps; every piece is its own code.  Its MaskField (n_layer=4, n_dim=128, skips=[], mask_dim=K,
softmax) is attached to fields A (K = 8) and B (K = 3; the same trunk, its own head) of the existing fixtures and the camera of the render_eval
goldens (make_golden.camera_rays: 16 x 16 rays, every second one) is rendered in eval mode through its NVFi.render_ray.  Hooks on the field's own modules record, per
render, the warped points its density is looked up at (the argument of compute_densityfeature), the colours its renderModule returns and the masks
its mask_field returns; the layer maps are composited here in torch fp32 from those and the render's own weights by the contract's formulas
(tests/objects64.py).  A SELECTED render is the same call with what the reference's feature2density returns scaled by s(x) = sum_k select_k
mask_field(x)_k at those warped points, inside this script.
The random-init MaskField gives nearly uniform masks: its last layer's weights are multiplied by HEAD_SCALE[kind] (recorded) so that the masks are
peaked and removing an object changes the image visibly (asserted: the removal cases move rgb by more than 0.02 somewhere).

Writes tests/golden/objects.npz (numbers only): per field <kind>:mask:<state_dict key>, <kind>:K, <kind>:head_scale; per case <kind>:<case>:{t,
select, rgb, depth, acc, weight, mask_map, obj_rgb, obj_acc, obj_depth, floor (3), max_abs (3), n_near, n_aside, M}.
  floor    max |objects64(float32) - objects64(float64)| / max |objects64(float64)| per layer map on the golden weights, not below one fp32 ulp of the
           map scale: the plain-fp32 noise floor the bounds of tests/test_objects_golden.py and tests/test_gpu_objects.py are derived from
  n_aside  rays the yardstick's own float32 run leaves outside the map rule (objects64.map_failures); ASSERTED to be rays of the near-threshold
           report and at most 2 % of the case's rays (a case that needs more is replaced, the cap is not raised)
Cases: times k (a keyframe time), n (19/60, not a keyframe), x (past the last keyframe: extrapolated); select o (all ones), r (the dominant
object removed) at every time, i (the second-largest object alone) and f (fractions) at the non-key time.  Rays: every second one of the bundle."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import objects64 as o64  # noqa: E402
import render64 as r64  # noqa: E402

HEAD_SCALE = {"A": 150.0, "B": 40.0}
T_NONKEY = 19.0 / 60.0
FLOORS = {"rgb": 2e-6, "acc": 2e-6, "depth": 2e-5, "weight": 2e-6}      # helpers.FP32_FLOOR


class Tap:
    """records what the reference's own modules see and return during one render, and scales feature2density's result by s(x)"""

    def __init__(self, f):
        self.f, self.select = f, None
        self.x = self.rgb = self.mask = None
        self.inside = False
        dens, f2d = f.compute_densityfeature, f.feature2density

        def density(xyzt, *a, **k):
            self.x = xyzt[..., :3].detach().clone()
            return dens(xyzt, *a, **k)

        def to_density(feat, *a, **k):
            sig = f2d(feat, *a, **k)
            if self.select is not None:
                self.inside = True
                sig = sig * (f.mask_field(self.x) * self.select).sum(-1)
                self.inside = False
            return sig

        f.compute_densityfeature, f.feature2density = density, to_density
        f.renderModule.register_forward_hook(lambda m, i, o: setattr(self, "rgb", o.detach().clone()))

    def attach(self, mf):
        self.f.mask_field = mf
        mf.register_forward_hook(lambda m, i, o: None if self.inside else setattr(self, "mask", o.detach().clone()))


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    from helpers import load_meta
    torch.manual_seed(4242)
    mfA = R["MaskField"](n_layer=4, n_dim=128, skips=[], mask_dim=8, input_dim=3, mask_act="softmax")
    mfB = R["MaskField"](n_layer=4, n_dim=128, skips=[], mask_dim=3, input_dim=3, mask_act="softmax")
    mfB.point_fc.load_state_dict(mfA.point_fc.state_dict())        # one trunk in the fixture, two heads
    with torch.no_grad():
        mfA.mask_fc.weight.mul_(HEAD_SCALE["A"])
        mfB.mask_fc.weight.mul_(HEAD_SCALE["B"])
    fx, floors = {}, {}
    for kind, cfg, nv, mf in (("A", cfgA, nvA, mfA), ("B", cfgB, nvB, mfB)):
        f = nv.nvfi
        f.eval()
        mf.eval()
        K = mf.mask_dim
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        mparams = o64.mask_params(mf.state_dict())
        fx[f"{kind}:K"], fx[f"{kind}:head_scale"] = np.int64(K), np.float64(HEAD_SCALE[kind])
        for k, v in mf.state_dict().items():
            if kind == "A" or k.startswith("mask_fc"):
                fx[f"{kind}:mask:{k}"] = mg.npf(v)
        tap = Tap(f)
        tap.attach(mf)
        o, d = mg.camera_rays(R, kind)
        o, d = o[::2].contiguous(), d[::2].contiguous()        # every second ray of the 16 x 16 bundle: the fixture stays under the size limit
        white = bool(cfg.dataset.white_background)
        ts = f.tmax / (f.num_keyframes - 1)
        thres = f.rayMarch_weight_thres
        nR = o.shape[0]

        def render(t, select):
            tap.select = None if select is None else torch.as_tensor(select, dtype=torch.float32)
            with torch.no_grad():
                rgb, depth, acc, weight, mask_map = nv.render_ray(t, o, d, white, False)     # (its Renderer reshapes the fifth output to 3 channels)
                weight = weight.reshape(nR, -1)
                _, z, _ = f.sample_ray(o, d)
                am = weight > thres
                ray = am.nonzero()[:, 0]
                assert tap.rgb.shape[0] == tap.mask.shape[0] == int(am.sum()), (tap.rgb.shape, tap.mask.shape, int(am.sum()))
                wm = weight[am][:, None] * tap.mask                                         # (M, K)
                obj_acc = torch.zeros(nR, K).index_add(0, ray, wm)
                obj_rgb = torch.zeros(nR, K, 3).index_add(0, ray, wm[:, :, None] * tap.rgb[:, None, :])
                obj_depth = torch.zeros(nR, K).index_add(0, ray, wm * z[am][:, None])
            return dict(rgb=rgb.reshape(nR, 3), depth=depth.reshape(nR), acc=acc.reshape(nR), weight=weight, mask_map=mask_map.reshape(nR, K),
                        obj_rgb=obj_rgb, obj_acc=obj_acc, obj_depth=obj_depth)

        rng = np.random.default_rng(5 if kind == "A" else 6)
        for tn, t in (("k", 2 * ts), ("n", T_NONKEY), ("x", f.tmax + 0.7 * ts)):
            plain = render(t, None)
            dom = int(plain["obj_acc"].sum(0).argmax())
            ones = np.ones(K, np.float32)
            rem, iso = ones.copy(), np.zeros(K, np.float32)
            rem[dom], iso[int(plain["obj_acc"].sum(0).argsort()[-2])] = 0.0, 1.0
            frac = np.round(rng.uniform(0.2, 0.9, K), 2).astype(np.float32)
            print(f"{kind}:{tn}: t={t:.4f} dominant object {dom}, mean max_k mask {float(tap.mask.max(1).values.mean()):.3f}, "
                  f"share of acc per object {np.round((plain['obj_acc'].sum(0) / plain['obj_acc'].sum()).numpy(), 3)}")
            for sn, sel in (("o", ones), ("r", rem), ("i", iso), ("f", frac)) if tn == "n" else (("o", ones), ("r", rem)):
                key = f"{kind}:{tn}{sn}"
                ref = render(t, sel)
                y64 = o64.objects64(field, mparams, o.numpy(), d.numpy(), t, white, select=sel, weights=ref["weight"].numpy())
                y32 = o64.objects64(field, mparams, o.numpy(), d.numpy(), t, white, select=sel, weights=ref["weight"].numpy(), dtype=torch.float32)
                fl = o64.layer_floor(y32, y64)
                bad = o64.map_failures(y32, y64, FLOORS)
                aside = np.unique(np.concatenate([v for v in bad.values()])) if bad else np.zeros(0, np.int64)
                near = np.union1d(y64["near_rays"], y32["near_rays"])
                assert np.isin(aside, near).all(), (key, "fp32 yardstick fails away from the threshold", bad)
                assert len(aside) <= o64.MAX_ASIDE * nR, (key, "needs more than 2 % of its rays set aside: replace the case", len(aside))
                fx[key + ":t"], fx[key + ":select"] = np.float64(t), sel
                for k, v in ref.items():
                    fx[f"{key}:{k}"] = mg.npf(v)
                fx[key + ":floor"] = np.array(fl)
                fx[key + ":max_abs"] = np.array([np.abs(y64[k]).max() for k in o64.LAYER_KEYS])
                fx[key + ":n_near"], fx[key + ":n_aside"], fx[key + ":M"] = np.int64(len(near)), np.int64(len(aside)), np.int64(y64["M"])
                floors[key] = fl
                ref_err = [o64.rel_err(ref[k].numpy(), y64[k]) for k in o64.LAYER_KEYS]
                move = float((ref["rgb"] - plain["rgb"]).abs().max())
                print(f"{key}: select={sel} M={y64['M']} floor={np.array(fl)} reference-vs-yardstick={np.array(ref_err)} near rays {len(near)} "
                      f"set aside {len(aside)} max |rgb - plain rgb| {move:.3f}")
                if sn in "ri":
                    assert move > 0.02, (key, "the selection does not change the image", move)
                assert fx[key + ":max_abs"].min() > 1e-3 or sn == "i", (key, fx[key + ":max_abs"])
    path = os.path.join(HERE, "objects.npz")
    np.savez_compressed(path, **fx)
    print("wrote objects.npz", os.path.getsize(path), "bytes")
    print("GOLDEN_FLOOR = {")
    for k, fl in floors.items():
        print(f'    "{k}": ({", ".join(f"{x:.1e}" for x in _up(fl))}),')
    print("}")


def _up(fl):
    """rounded UP to two digits"""
    out = []
    for x in fl:
        e = int(np.floor(np.log10(x)))
        out.append(np.ceil(x / 10.0 ** (e - 1)) * 10.0 ** (e - 1))
    return out


if __name__ == "__main__":
    main()
