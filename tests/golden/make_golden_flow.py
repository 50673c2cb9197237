#!/usr/bin/env python
"""Golden vectors of the flow branch (nvfi_render_flow), generated from the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_flow.py        (NVFI_REFERENCE: checkout of the reference; default as in make_golden.py)
The reference has no call that renders these maps; every piece is its own code: the weights of its test-mode Renderer.render on the camera of
the render_eval goldens (make_golden.camera_rays: 16 x 16 rays of an 800 x 800 camera), its sample_ray / normalize_coord for the un-warped
positions, field.vel (VelocityAABB[Sur].forward) and field.integrate_pos at the appearance-masked samples, composited here in torch fp32 by the
contract's formulas (tests/flow64.py).  Writes tests/golden/flow.npz (numbers only): per case <kind>:<case>:{t, dt, transfer, wkey (names the weight map), vel_map,
flow_map, flow2d, max_abs (3), floor (3), n_rejected, M}, and per field <kind>:{pose, H, W, focal}.
  floor       max |flow64(float32) - flow64(float64)| / max |flow64(float64)| per map, on the golden weights: the plain-fp32 noise floor the
              bounds of tests/test_flow_golden.py and tests/test_gpu_flow.py are derived from
  n_rejected  steps of points inside the surround box that the box rejected (field B), counted by the yardstick
It ASSERTS what makes the cases well-posed: no masked sample within 4 fp32 ulp of a gate or box face (flow64's edge report), max |map| of
every non-zero case above 1e-3 of its natural scale (the signal is there), and at least one rejected step in the case that is there for it.

Cases (ts = tmax / (K - 1)):  c1 non-key t, dt = +ts/4 (one step) | c2 non-key t, dt = -1.3 ts (two full steps and a remainder) | c3 key t,
dt = +ts/2 | c4 t = 45/60, dt = +0.2 (leaves tmax) | c5 non-key t, dt = +ts/4 on the weights of a transfer_vel render | c6 dt = 0 |
c7 (field B only) non-key t, the first dt of a fixed list whose integration has a rejected step."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import flow64 as f64  # noqa: E402
import render64 as r64  # noqa: E402

T_NONKEY = 19.0 / 60.0


def reference_maps(f, o, d, weight, t, dt, pose, focal):
    """the three maps from the reference's own field calls, fp32"""
    thres = f.rayMarch_weight_thres
    with torch.no_grad():
        pts, _, _ = f.sample_ray(o, d)
        x = f.normalize_coord(pts)
        mask = weight > thres
        ray = mask.nonzero()[:, 0]
        xm, w = x[mask], weight[mask]
        tt = torch.full_like(xm[:, :1], float(t))
        half = (f.aabb[1] - f.aabb[0]) / 2
        v = f.vel(torch.cat([xm, tt], -1))
        xd = f.integrate_pos(xm.clone(), tt.clone(), tt.clone() + float(dt))
        R = o.shape[0]

        def seg(val):
            return torch.zeros(R, val.shape[1]).index_add(0, ray, w[:, None] * val)

        def pix(xn):
            P = f.aabb[0] + (xn + 1) * half
            c = (P - pose[:3, 3]) @ pose[:3, :3]
            return torch.stack([focal * c[:, 0] / -c[:, 2], -(focal * c[:, 1] / -c[:, 2])], 1), -c[:, 2]

        p0, _ = pix(xm)
        p1, z1 = pix(xd)
        d2 = torch.where((z1 < 1e-3)[:, None], torch.zeros_like(p0), p1 - p0)
        return seg(half * v), seg(half * (xd - xm)), seg(d2)


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    sys.path.insert(0, os.path.dirname(HERE))
    from helpers import load_meta
    fx = {}
    for kind, cfg, nv in (("A", cfgA, nvA), ("B", cfgB, nvB)):
        f = nv.nvfi
        f.eval()
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        ren = R["Renderer"](nv, 0, 0, 2048)
        o, d = mg.camera_rays(R, kind)
        full = 800
        pose = mg.pose_spherical(30.0, -30.0, 4.0, (0, 0, 0) if kind == "A" else (0.0, 0.0, 3.0))[:3, :4].contiguous()
        focal = float(np.float32(0.5 * full / np.tan(0.5 * 0.6911112)))
        fx[f"{kind}:pose"], fx[f"{kind}:H"], fx[f"{kind}:W"], fx[f"{kind}:focal"] = mg.npf(pose), np.int64(full), np.int64(full), np.float32(focal)
        ts = f.tmax / (f.num_keyframes - 1)
        cases = [("c1", T_NONKEY, ts / 4, False), ("c2", T_NONKEY, -1.3 * ts, False), ("c3", 2 * ts, ts / 2, False),
                 ("c4", 45.0 / 60.0, 0.2, False), ("c5", T_NONKEY, ts / 4, True), ("c6", T_NONKEY, 0.0, False)]
        if kind == "B":
            cases.append(("c7", T_NONKEY, None, False))
        for name, t, dt, transfer in cases:
            with torch.no_grad():
                weight = ren.render(t, R["Ray"](o, d, 0, 1), white_background=cfg.dataset.white_background, mode="test", transfer_vel=transfer)[3]
            weight = weight.reshape(o.shape[0], -1)
            cam = (pose.numpy(), full, full, focal)
            if dt is None:     # c7: the first dt with a rejected step
                for cand in (1.5 * ts, -1.5 * ts, 2.5 * ts, -2.5 * ts, 4.5 * ts, -4.5 * ts):
                    if f64.flow64(field, o.numpy(), d.numpy(), t, cand, weight.numpy(), None, want=("flow",))["n_rejected"] > 0:
                        dt = cand
                        break
                assert dt is not None, "no dt of the list gives a rejected step on field B"
            y64 = f64.flow64(field, o.numpy(), d.numpy(), t, dt, weight.numpy(), cam)
            y32 = f64.flow64(field, o.numpy(), d.numpy(), t, dt, weight.numpy(), cam, dtype=torch.float32)
            assert len(y64["edge_samples"]) == 0 and len(y32["edge_samples"]) == 0, (kind, name, y64["edge_samples"])
            vm, fm, f2 = reference_maps(f, o, d, weight, t, dt, pose, focal)
            key = f"{kind}:{name}"
            fx[key + ":t"], fx[key + ":dt"], fx[key + ":transfer"] = np.float64(t), np.float64(dt), np.int64(transfer)
            wkey = f"{kind}:weight:{'transfer' if transfer else 'plain'}:{t:.6f}"       # cases at the same time share their render
            fx[wkey] = mg.npf(weight)
            fx[key + ":wkey"] = np.array(wkey)
            fx[key + ":vel_map"], fx[key + ":flow_map"], fx[key + ":flow2d"] = mg.npf(vm), mg.npf(fm), mg.npf(f2)
            mx = np.array([np.abs(y64[k]).max() for k in ("vel_map", "flow_map", "flow2d")])
            fl = np.array([f64.rel_err(y32[k], y64[k]) for k in ("vel_map", "flow_map", "flow2d")])
            fx[key + ":max_abs"], fx[key + ":floor"] = mx, fl
            fx[key + ":n_rejected"], fx[key + ":M"] = np.int64(y64["n_rejected"]), np.int64(y64["M"])
            ref_err = [f64.rel_err(g, y64[k]) for g, k in ((vm, "vel_map"), (fm, "flow_map"), (f2, "flow2d"))]
            print(f"{key}: t={t:.4f} dt={dt:+.4f} M={y64['M']} steps={len(y64['steps'])} rejected={y64['n_rejected']} max|map|={mx} "
                  f"floor(fp32 yardstick)={fl} reference-vs-yardstick={ref_err}")
            assert mx[0] > 1e-3, (key, mx)
            if dt != 0:
                assert mx[1] > 1e-3 * abs(dt) and mx[2] > 1e-3, (key, mx)
            if name == "c7":
                assert y64["n_rejected"] >= 1
    np.savez_compressed(os.path.join(HERE, "flow.npz"), **fx)
    print("wrote flow.npz", os.path.getsize(os.path.join(HERE, "flow.npz")), "bytes")


if __name__ == "__main__":
    main()
