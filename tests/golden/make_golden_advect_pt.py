#!/usr/bin/env python
"""Golden vectors of differentiable advection with PER-POINT times (nvfi_advect_grad_pt / TensorVMKeyframeTimeKplane.advect_pt), generated from
the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_advect_pt.py        (the checkout of the reference as in make_golden.py)
The reference's integrate_pos (models/tensorf_keyframe.py:575-611) is plain torch code over (N,1) time tensors; autograd carries a loss on the
advected points back to the input points and to vel_net.weight_net for any mix of times.  Per case, eval mode, exactly as
make_golden_advect.py: reference_run but with per-point tensors:
    y = f.integrate_pos(x * 1.0, tt.clone(), bb.clone());  (y * g).sum().backward()          tt, bb (N,1)
Cases, fields A and B (advect_pt64.case_of):
    mixed      N = 257, advect64.case_inputs(257), the five time pairs of make_golden_advect.py: cases_of(kind, ts) assigned by i % 5
    distinct   N = 97, advect64.case_inputs(97), rng = default_rng(1257), t = rng.random(97) * tmax, t_target = t + (rng.random(97) * 4.4 - 2.2) * ts,
               rounded to fp32: 97 distinct pairs
Writes (numbers only; every file under 1 MiB):
    advect_pt.npz            <kind>:<case>:{t, t_target (N, fp32), x, g, xk, gx, steps (N), n_rejected, n_outside, floor (xk, gx, worst net tensor)}
    advect_pt_net_<kind>.npz <kind>:<case>:<parameter name>, both cases of a field
It ASSERTS what makes the cases well-posed: no point within 4 fp32 ulp of a gate or box face at any evaluation in float64 or float32 (the
yardstick's edge report), the same rejected steps in both precisions, the step counts of the mixed case ({0, 1, 3, 2, 8} on A, {0, 1, 3, 8, 9}
on B, rejected steps on B), 1 .. 5 steps in the distinct case, max |gx| above 1e-3 and every net gradient with a max above 1e-3, and that
a_weight_net receives nothing."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import advect64 as a64  # noqa: E402
import advect_pt64 as p64  # noqa: E402
import render64 as r64  # noqa: E402


def reference_run(f, x, g, t, t1):
    """xk, gx and the 12 parameter gradients from the reference's own integrate_pos under autograd, fp32, per-point times"""
    for p in f.vel_net.parameters():
        p.grad = None
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    tt = torch.from_numpy(t).reshape(-1, 1).clone()
    bb = torch.from_numpy(t1).reshape(-1, 1).clone()
    y = f.integrate_pos(xt * 1.0, tt.clone(), bb.clone())
    (y * torch.from_numpy(g)).sum().backward()
    named = dict(f.named_parameters())
    net = {k: (named[k].grad.clone() if named[k].grad is not None else torch.zeros_like(named[k])) for k in a64.NET_NAMES}
    a_net_touched = any(named[k].grad is not None and bool(named[k].grad.abs().max() > 0) for k in named if k.startswith("vel_net.a_weight_net"))
    return mg.npf(y), mg.npf(xt.grad), {k: mg.npf(v) for k, v in net.items()}, a_net_touched


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
        f.eval()
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        ts = f.tmax / (f.num_keyframes - 1)
        for name in ("mixed", "distinct"):
            key = f"{kind}:{name}"
            x, g, t, t1 = p64.case_of(kind, name, f.tmax, ts)
            y64 = p64.advect_pt64(field, x, t, t1, g)
            y32 = p64.advect_pt64(field, x, t, t1, g, dtype=torch.float32)
            assert not y64["edge"].any() and not y32["edge"].any(), (key, np.nonzero(y64["edge"] | y32["edge"])[0])
            assert y64["n_rejected"] == y32["n_rejected"], key
            if name == "mixed":
                assert list(y64["steps"][:5]) == ([0, 1, 3, 2, 8] if kind == "A" else [0, 1, 3, 8, 9]), (key, y64["steps"][:5])
                assert kind == "A" or y64["n_rejected"] > 0, key
            else:
                assert y64["groups"] == len(x) and y64["steps"].min() >= 1 and y64["steps"].max() <= 5, (key, y64["groups"], y64["steps"])
            xk, gx, net, a_touched = reference_run(f, x, g, t, t1)
            assert not a_touched, key
            fl = np.array(a64.floors(y32, y64))
            fx[key + ":t"], fx[key + ":t_target"] = t, t1
            fx[key + ":x"], fx[key + ":g"], fx[key + ":xk"], fx[key + ":gx"] = x, g, xk, gx
            fx[key + ":steps"], fx[key + ":n_rejected"], fx[key + ":n_outside"] = y64["steps"], np.int64(y64["n_rejected"]), np.int64(y64["n_outside"])
            fx[key + ":floor"] = fl
            ref_err = (a64.flow64.rel_err(xk, y64["xk"]), a64.flow64.rel_err(gx, y64["gx"]), max(a64.flow64.rel_err(net[k], y64[k]) for k in a64.NET_NAMES))
            print(f"{key}: N={len(x)} pairs={y64['groups']} steps={sorted(set(y64['steps'].tolist()))} outside={y64['n_outside']} rejected={y64['n_rejected']} "
                  f"floor(fp32 yardstick; xk, gx, worst net)={fl} reference-vs-yardstick={ref_err}")
            small = min(float(np.abs(v).max()) for v in net.values())
            print(f"    max |gx| {np.abs(gx).max():.3g}, smallest max |net gradient| {small:.3g}")
            assert np.abs(gx).max() > 1e-3 and small > 1e-3, (key, {k: float(np.abs(v).max()) for k, v in net.items()})
            dst = nets.setdefault(f"advect_pt_net_{kind}.npz", {})
            for k, v in net.items():
                dst[f"{key}:{k}"] = v
    np.savez_compressed(os.path.join(HERE, "advect_pt.npz"), **fx)
    print("wrote advect_pt.npz", os.path.getsize(os.path.join(HERE, "advect_pt.npz")), "bytes")
    for fn, d in nets.items():
        np.savez_compressed(os.path.join(HERE, fn), **d)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
        assert os.path.getsize(os.path.join(HERE, fn)) < (1 << 20), fn


if __name__ == "__main__":
    main()
