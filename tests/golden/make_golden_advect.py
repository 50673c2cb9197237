#!/usr/bin/env python
"""Golden vectors of differentiable advection (nvfi_advect_grad / TensorVMKeyframeTimeKplane.advect), generated from the REFERENCE implementation
(PyTorch CPU):
    python tests/golden/make_golden_advect.py        (the checkout of the reference as in make_golden.py)
The reference's integrate_pos (models/tensorf_keyframe.py:575-611) is plain torch code; autograd carries a loss on the advected points back to
the input points and to vel_net.weight_net.  Per case, eval mode:
    y = f.integrate_pos(x * 1.0, tt.clone(), bb.clone());  (y * g).sum().backward()
Fields A and B, N = 257, x = rng.random((N, 3)) * 2.1 - 1.05 and g = rng.standard_normal((N, 3)) with rng = default_rng(11 + N)
(advect64.case_inputs), T = 19/60, ts = tmax / (K - 1).  Cases:
    c0 t == t_target (no step) | c1 T -> T + ts/4 (one step) | c2 T -> T - 1.3 ts (three) | c3 45/60 -> +0.2 (leaves tmax: 2 steps on A, 8 on B) |
    c4 0 -> 1.0 on A (8 steps), 0 -> 4.5 ts on B (9 steps)
Writes (numbers only; a committed file stays under 1 MiB, so the 12 net gradients of two cases each go to a file of their own):
    advect.npz              <kind>:<case>:{t, t_target, x, g, xk, gx, steps, n_rejected, n_outside, floor (xk, gx, worst net tensor)}, and the replay
                            record replay:{x, target, t, t_target, loss (3), <the 12 final parameters>}
    advect_net_<kind><n>.npz  <kind>:<case>:<parameter name> for the cases c1, c2 (n = 1) and c3, c4 (n = 2); c0's gradients are exact zeros
  floor       max |advect64(float32) - advect64(float64)| / max |advect64(float64)|: the plain-fp32 noise floor the bounds of
              tests/test_advect_golden.py and tests/test_gpu_advect.py are derived from
It ASSERTS what makes the cases well-posed: no point within 4 fp32 ulp of a gate or box face at any evaluation (advect64's edge report), rejected
steps in the three cases of field B that are there for them (c2, c3, c4), max |gx| above 1e-3 and every net gradient with a max above 1e-3 per
unit of advection time (all but three tensors of B:c1, whose step is 0.0125, are above 1e-3 outright), and that a_weight_net
receives nothing.  Replay record: three iterations of torch.optim.Adam(weight_net, lr 1e-3) on mean((integrate_pos(x) - target)^2), target = x
rotated by 0.1 rad about z, field A, N = 257, the one-step pair of c1."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import advect64 as a64  # noqa: E402
import render64 as r64  # noqa: E402

T_NONKEY = 19.0 / 60.0
N = 257


def cases_of(kind, ts):
    return [("c0", T_NONKEY, T_NONKEY), ("c1", T_NONKEY, T_NONKEY + ts / 4), ("c2", T_NONKEY, T_NONKEY - 1.3 * ts), ("c3", 45.0 / 60.0, 45.0 / 60.0 + 0.2),
            ("c4", 0.0, 1.0 if kind == "A" else 4.5 * ts)]


def reference_run(f, x, g, t, t1):
    """xk, gx and the 12 + 12 parameter gradients from the reference's own integrate_pos under autograd, fp32"""
    for p in f.vel_net.parameters():
        p.grad = None
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    tt = torch.full((x.shape[0], 1), float(t))
    bb = torch.full((x.shape[0], 1), float(t1))
    y = f.integrate_pos(xt * 1.0, tt.clone(), bb.clone())
    loss = (y * torch.from_numpy(g)).sum()
    if loss.requires_grad:
        loss.backward()
    named = dict(f.named_parameters())
    gx = xt.grad if xt.grad is not None else torch.from_numpy(g).clone()
    net = {k: (named[k].grad.clone() if named[k].grad is not None else torch.zeros_like(named[k])) for k in a64.NET_NAMES}
    a_net_touched = any(named[k].grad is not None and bool(named[k].grad.abs().max() > 0) for k in named if k.startswith("vel_net.a_weight_net"))
    return mg.npf(y), mg.npf(gx), {k: mg.npf(v) for k, v in net.items()}, a_net_touched


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    from helpers import load_meta
    fx, nets = {}, {}
    x, g = a64.case_inputs(N)
    for kind, nv in (("A", nvA), ("B", nvB)):
        f = nv.nvfi
        f.eval()
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        ts = f.tmax / (f.num_keyframes - 1)
        for name, t, t1 in cases_of(kind, ts):
            key = f"{kind}:{name}"
            y64 = a64.advect64(field, x, t, t1, g)
            y32 = a64.advect64(field, x, t, t1, g, dtype=torch.float32)
            assert not y64["edge"].any() and not y32["edge"].any(), (key, np.nonzero(y64["edge"])[0])
            assert y64["n_rejected"] == y32["n_rejected"], key
            xk, gx, net, a_touched = reference_run(f, x, g, t, t1)
            assert not a_touched, key
            fl = np.array(a64.floors(y32, y64))
            fx[key + ":t"], fx[key + ":t_target"] = np.float64(t), np.float64(t1)
            fx[key + ":x"], fx[key + ":g"], fx[key + ":xk"], fx[key + ":gx"] = x, g, xk, gx
            fx[key + ":steps"], fx[key + ":n_rejected"], fx[key + ":n_outside"] = np.int64(len(y64["steps"])), np.int64(y64["n_rejected"]), np.int64(y64["n_outside"])
            fx[key + ":floor"] = fl
            ref_err = (a64.flow64.rel_err(xk, y64["xk"]), a64.flow64.rel_err(gx, y64["gx"]), max(a64.flow64.rel_err(net[k], y64[k]) for k in a64.NET_NAMES))
            print(f"{key}: t={t:.4f} -> {t1:.4f} steps={len(y64['steps'])} outside={y64['n_outside']} rejected={y64['n_rejected']} "
                  f"floor(fp32 yardstick; xk, gx, worst net)={fl} reference-vs-yardstick={ref_err}")
            if name == "c0":
                assert np.array_equal(xk, x) and np.array_equal(gx, g) and all(not v.any() for v in net.values()), key
                continue
            if kind == "B" and name in ("c2", "c3", "c4"):
                assert y64["n_rejected"] > 0, key
            # the signal is there: gx is of the size of g; a net gradient is proportional to the advection time to first order, so its floor is
            # 1e-3 per unit of time, as make_golden_flow.py scales its flow maps (B:c1, a step of ts/4 = 0.0125, has three tensors at 6.5e-4 .. 8.9e-4)
            small = min(float(np.abs(v).max()) for v in net.values())
            print(f"    max |gx| {np.abs(gx).max():.3g}, smallest max |net gradient| {small:.3g}")
            assert np.abs(gx).max() > 1e-3 and small > 1e-3 * abs(t1 - t), (key, {k: float(np.abs(v).max()) for k, v in net.items()})
            dst = nets.setdefault(f"advect_net_{kind}{1 if name in ('c1', 'c2') else 2}.npz", {})
            for k, v in net.items():
                dst[f"{key}:{k}"] = v
    # the replay record: three Adam iterations of the reference on a copy of field A
    f = copy.deepcopy(nvA).nvfi
    f.eval()
    ts = f.tmax / (f.num_keyframes - 1)
    t, t1 = T_NONKEY, T_NONKEY + ts / 4
    c, s = float(np.cos(np.float32(0.1))), float(np.sin(np.float32(0.1)))
    xt = torch.from_numpy(x)
    target = torch.stack([c * xt[:, 0] - s * xt[:, 1], s * xt[:, 0] + c * xt[:, 1], xt[:, 2]], 1)
    opt = torch.optim.Adam(f.vel_net.weight_net.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        y = f.integrate_pos(xt * 1.0, torch.full((N, 1), float(t)), torch.full((N, 1), float(t1)))
        loss = ((y - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    fx["replay:x"], fx["replay:target"], fx["replay:t"], fx["replay:t_target"] = x, mg.npf(target), np.float64(t), np.float64(t1)
    fx["replay:loss"] = np.array(losses, np.float64)
    named = dict(f.named_parameters())
    for k in a64.NET_NAMES:
        fx["replay:" + k] = mg.npf(named[k])
    print("replay losses", losses)
    np.savez_compressed(os.path.join(HERE, "advect.npz"), **fx)
    print("wrote advect.npz", os.path.getsize(os.path.join(HERE, "advect.npz")), "bytes")
    for fn, d in nets.items():
        np.savez_compressed(os.path.join(HERE, fn), **d)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main()
