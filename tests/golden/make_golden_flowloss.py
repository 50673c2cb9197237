#!/usr/bin/env python
"""Golden vectors of the optical-flow loss (nvfi_flow_loss_fwd / nvfi_flow_loss_bwd; TensorVMKeyframeTimeKplane.flow_loss), generated from the
REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_flowloss.py        (the checkout of the reference as in make_golden.py)
The reference has no such term; every piece is its own code.  Per field (A, B; those of the 16 x 16 rays of make_golden.camera_rays whose samples keep 4 fp32 ulp from every decision in every case):
  - a TRAIN-mode forward with a fixed jitter (torch.manual_seed(11) in front of the draw of sample_ray, as make_golden.py fixes sample_train:u)
    for the weights, and the same draw again for its sample_ray / normalize_coord: the un-warped positions x_j of the masked samples;
  - its integrate_pos under autograd, in eval mode as make_golden_advect.py runs it, on the x_j; then the projection, the composite and the
    loss of the contract (tests/flowloss64.py) in torch fp32, and backward: g_weights and the 12 gradients of vel_net.weight_net.
Cases (ts = tmax / (K - 1), T = 19/60, target = default_rng(21).standard_normal((R, 2)) * 3):
    c0 dt = 0 | c1 dt = +ts/4 (one step) | c2 dt = -1.3 ts (three) | c3 c1 with kind = huber, delta = 2 | c4 c1 with a valid mask that has zeros and two
    NaN targets | c5 c1 with no valid ray | c6 c1 projected by a camera placed INSIDE the box: displaced samples fall behind the -c_z = 1e-3 guard
Writes (numbers only, each file under 1 MiB):
    flowloss.npz             <kind>:{rays_o, rays_d, u, weight, pose, pose_in, H, W, focal, target, valid4} and <kind>:<case>:{dt, kind, delta, flow2d, loss,
                             n, g_weights, M, n_guard, n_rejected, floor (flow2d, loss, g_weights, worst net tensor)}
    flowloss_net_<kind><n>.npz  <kind>:<case>:<parameter name> for c1, c2, c3 (n = 1) and c4, c6 (n = 2); c0 and c5 are exact zeros
It ASSERTS what makes the cases well-posed: no masked sample within 4 fp32 ulp of a gate face, a box face or the guard (flowloss64's edge
report, float64 and float32 runs), entries behind the guard in c6 and none elsewhere, and that a_weight_net receives nothing."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import flow64 as f64  # noqa: E402
import flowloss64 as fl64  # noqa: E402
import render64 as r64  # noqa: E402

T_NONKEY = 19.0 / 60.0
SEED = 11


def reference_run(f, x, weight, t, dt, pose, focal, target, valid, kind, delta):
    """flow2d, loss, n, g_weights and the 12 + 12 parameter gradients from the reference's own integrate_pos under autograd on its own sample
    positions x (R, S, 3), fp32"""
    for p in f.vel_net.parameters():
        p.grad = None
    f.eval()
    mask = weight > f.rayMarch_weight_thres
    ray = mask.nonzero()[:, 0]
    xm = x[mask]
    w = weight[mask].clone().requires_grad_(True)
    tt = torch.full_like(xm[:, :1], float(t))
    xd = f.integrate_pos(xm * 1.0, tt.clone(), tt.clone() + float(dt))
    half = (f.aabb[1] - f.aabb[0]) / 2

    def pix(xn):
        P = f.aabb[0] + (xn + 1) * half
        c = (P - pose[:3, 3]) @ pose[:3, :3]
        return torch.stack([focal * c[:, 0] / -c[:, 2], -(focal * c[:, 1] / -c[:, 2])], 1), -c[:, 2]

    p0, _ = pix(xm)
    p1, z1 = pix(xd)
    d2 = torch.where((z1.detach() < 1e-3)[:, None], torch.zeros_like(p0), p1 - p0)
    R = x.shape[0]
    flow2d = torch.zeros(R, 2).index_add(0, ray, w[:, None] * d2)
    ok = torch.isfinite(target).all(-1) & (valid != 0)
    e = flow2d - torch.where(ok[:, None], target, torch.zeros_like(target))
    rho = e * e if kind == "l2" else F.huber_loss(e, torch.zeros_like(e), reduction="none", delta=delta)
    n = int(ok.sum())
    loss = (rho * ok[:, None]).sum() / (2 * n) if n > 0 else (flow2d * 0).sum()
    loss.backward()
    named = dict(f.named_parameters())
    gw = torch.zeros_like(weight)
    gw[mask] = w.grad
    net = {k: (named[k].grad.clone() if named[k].grad is not None else torch.zeros_like(named[k])) for k in fl64.NET_NAMES}
    a_touched = any(named[k].grad is not None and bool(named[k].grad.abs().max() > 0) for k in named if k.startswith("vel_net.a_weight_net"))
    return mg.npf(flow2d), float(loss.detach()), n, mg.npf(gw), {k: mg.npf(v) for k, v in net.items()}, a_touched


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    from helpers import load_meta
    fx, nets = {}, {}
    for kind, nv in (("A", nvA), ("B", nvB)):
        f = nv.nvfi
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        o, d = mg.camera_rays(R, kind)
        Rn = o.shape[0]
        full = 800
        center = (0, 0, 0) if kind == "A" else (0.0, 0.0, 3.0)
        pose = mg.pose_spherical(30.0, -30.0, 4.0, center)[:3, :4].contiguous()
        pose_in = mg.pose_spherical(30.0, -30.0, 0.3, center)[:3, :4].contiguous()      # 0.3 from the box centre: inside, half the scene behind it
        focal = float(np.float32(0.5 * full / np.tan(0.5 * 0.6911112)))
        f.train()
        torch.manual_seed(SEED)
        u = torch.rand(Rn, 1)
        torch.manual_seed(SEED)
        with torch.no_grad():
            weight = f(T_NONKEY, o, d, white_bg=True)[3].reshape(Rn, -1)
            torch.manual_seed(SEED)
            pts, _, _ = f.sample_ray(o, d)
            x = f.normalize_coord(pts)
        f.eval()
        ts = f.tmax / (f.num_keyframes - 1)
        # rays: all whose samples keep 4 fp32 ulp from every decision in every case (the render is per ray: a subset keeps its rows)
        keep = np.ones(Rn, bool)
        for dt_, ps_ in ((ts / 4, pose), (-1.3 * ts, pose), (ts / 4, pose_in)):
            for dtype in (torch.float64, torch.float32):
                y = fl64.flowloss64(field, o.numpy(), d.numpy(), T_NONKEY, dt_, weight.numpy(), u.numpy().reshape(-1), (ps_.numpy(), full, full, focal),
                                    np.zeros((Rn, 2), np.float32), dtype=dtype)
                keep[y["idx"][y["edge"]][:, 0]] = False
        print(f"{kind}: {int((~keep).sum())} of {Rn} rays set aside (a sample within 4 ulp of a decision): {np.nonzero(~keep)[0]}")
        sel = torch.from_numpy(np.nonzero(keep)[0])
        o, d, u, weight, x = o[sel].contiguous(), d[sel].contiguous(), u[sel].contiguous(), weight[sel].contiguous(), x[sel].contiguous()
        Rn = len(sel)
        rng = np.random.default_rng(21)
        target = torch.from_numpy((rng.standard_normal((Rn, 2)) * 3).astype(np.float32))
        valid4 = torch.from_numpy((rng.random(Rn) < 0.7).astype(np.uint8))
        target4 = target.clone()
        target4[5, 0], target4[17, 1] = float("nan"), float("inf")
        ones, zeros = torch.ones(Rn, dtype=torch.uint8), torch.zeros(Rn, dtype=torch.uint8)
        pre = f"{kind}:"
        fx[pre + "rays_o"], fx[pre + "rays_d"], fx[pre + "u"], fx[pre + "weight"] = mg.npf(o), mg.npf(d), mg.npf(u), mg.npf(weight)
        fx[pre + "pose"], fx[pre + "pose_in"], fx[pre + "H"], fx[pre + "W"], fx[pre + "focal"] = mg.npf(pose), mg.npf(pose_in), np.int64(full), np.int64(full), np.float32(focal)
        fx[pre + "target"], fx[pre + "target4"], fx[pre + "valid4"] = mg.npf(target), mg.npf(target4), valid4.numpy()
        cases = [("c0", 0.0, "l2", 1.0, pose, target, ones), ("c1", ts / 4, "l2", 1.0, pose, target, ones), ("c2", -1.3 * ts, "l2", 1.0, pose, target, ones),
                 ("c3", ts / 4, "huber", 2.0, pose, target, ones), ("c4", ts / 4, "l2", 1.0, pose, target4, valid4), ("c5", ts / 4, "l2", 1.0, pose, target, zeros),
                 ("c6", ts / 4, "l2", 1.0, pose_in, target, ones)]
        for name, dt, lk, delta, ps, tg, vd in cases:
            key = f"{kind}:{name}"
            cam = (ps.numpy(), full, full, focal)
            a = (field, o.numpy(), d.numpy(), T_NONKEY, dt, weight.numpy(), u.numpy().reshape(-1), cam, tg.numpy())
            y64 = fl64.flowloss64(*a, valid=vd.numpy(), kind=lk, delta=delta)
            y32 = fl64.flowloss64(*a, valid=vd.numpy(), kind=lk, delta=delta, dtype=torch.float32)
            assert not y64["edge"].any() and not y32["edge"].any(), (key, np.nonzero(y64["edge"])[0])
            assert y64["n_rejected"] == y32["n_rejected"] and y64["n_guard"] == y32["n_guard"], key
            assert (y64["n_guard"] > 0) == (name == "c6"), (key, y64["n_guard"])
            flow2d, loss, n, gw, net, a_touched = reference_run(f, x, weight, T_NONKEY, dt, ps, focal, tg, vd, lk, delta)
            assert not a_touched and n == y64["n"], key
            fl = np.array(fl64.floors(y32, y64))
            fx[key + ":dt"], fx[key + ":kind"], fx[key + ":delta"] = np.float64(dt), np.array(lk), np.float64(delta)
            fx[key + ":flow2d"], fx[key + ":loss"], fx[key + ":n"], fx[key + ":g_weights"] = flow2d, np.float64(loss), np.int64(n), gw
            fx[key + ":M"], fx[key + ":n_guard"], fx[key + ":n_rejected"], fx[key + ":floor"] = np.int64(y64["M"]), np.int64(y64["n_guard"]), np.int64(y64["n_rejected"]), fl
            zero = name in ("c0", "c5")
            ref_err = (f64.rel_err(flow2d, y64["flow2d"]), abs(loss - y64["loss"]) / abs(y64["loss"]) if y64["loss"] else abs(loss),
                       f64.rel_err(gw, y64["g_weights"]), max(f64.rel_err(net[k], y64[k]) for k in fl64.NET_NAMES))
            print(f"{key}: dt={dt:+.4f} {lk} M={y64['M']} n={n} steps={len(y64['steps'])} guard={y64['n_guard']} rejected={y64['n_rejected']} loss={loss:.6g} "
                  f"floor(fp32 yardstick; flow2d, loss, g_weights, worst net)={fl} reference-vs-yardstick={ref_err}")
            if zero:
                assert not gw.any() and all(not v.any() for v in net.values()), key
                if name == "c0":
                    assert not flow2d.any()
                continue
            small = min(float(np.abs(v).max()) for v in net.values())
            print(f"    max |flow2d| {np.abs(flow2d).max():.3g}, max |g_weights| {np.abs(gw).max():.3g}, smallest max |net gradient| {small:.3g}")
            assert np.abs(flow2d).max() > 1e-2 and np.abs(gw).max() > 1e-3 and small > 1e-3 * abs(dt), key
            dst = nets.setdefault(f"flowloss_net_{kind}{1 if name in ('c1', 'c2', 'c3') else 2}.npz", {})
            for k, v in net.items():
                dst[f"{key}:{k}"] = v
    np.savez_compressed(os.path.join(HERE, "flowloss.npz"), **fx)
    print("wrote flowloss.npz", os.path.getsize(os.path.join(HERE, "flowloss.npz")), "bytes")
    for fn, dd in nets.items():
        np.savez_compressed(os.path.join(HERE, fn), **dd)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
