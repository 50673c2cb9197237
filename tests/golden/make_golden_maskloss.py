#!/usr/bin/env python
"""Golden vectors of the mask loss (nvfi_mask_loss_fwd / nvfi_mask_loss_bwd; TensorVMKeyframeTimeKplane.mask_loss), generated from the REFERENCE
implementation (PyTorch CPU):
    python tests/golden/make_golden_maskloss.py        (the checkout of the reference as in make_golden.py)
The reference has no such loss; its mask map is its own code.  Per field (A, B; the rays of tests/golden/flowloss.npz):
  - a TRAIN-mode forward of the reference's render_pts with its MaskField attached and a fixed jitter (torch.manual_seed(11) in front of the
    draw of sample_ray, as make_golden_flowloss.py fixes it): weight and mask_map with their autograd nodes;
  - the loss of the contract (tests/maskloss64.py) on that mask_map in torch fp32 and autograd.grad: the gradient of the ten MaskField tensors
    from the parameters, the gradient to `weight` from the returned weight node.
Cases (K = 8: the MaskField of tests/golden/maskfield.npz, tag K8; eps = 1e-5):
    c0 l2, labels | c1 ce, labels | c2 ce, soft rows | c3 ce, labels with ignored rays and a background label | c4 every ray ignored |
    c5 ce, labels, K = 17 (maskfield64.params_for(17))
Writes tests/golden/maskloss.npz (numbers only, under 1 MiB): <kind>:{u (the jitter drawn), ignored (rays left out of every case)} and <kind>:<case>:{kind, K, target,
mask_map, loss, n, g_weights (the masked entries of the counted rays, list order), M, floor (mask_map, loss, g_weights, worst of the ten)}, <kind>:{weight_masked,
mask (packed bits)}; and maskloss_grads_<kind><n>.npz: <kind>:<case>:<the ten gradients> for c0, c1, c2 (n = 1) and c3, c5 (n = 2); c4 is exact zeros.
It ASSERTS what makes the cases well-posed: every masked sample of the kept rays has maskfield64.margin >= KINK_MARGIN and a weight 4 fp32 ulp
away from the threshold; the others are ignored in every case (label -1 / a NaN row)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import maskfield64 as m64  # noqa: E402
import maskloss64 as ml64  # noqa: E402
import render64 as r64  # noqa: E402

T_NONKEY = 19.0 / 60.0
SEED = 11
EPS = 1e-5
N_RAYS = 256      # (all rays of the fixture when it holds fewer)


def attach(R, f, K):
    mf = R["MaskField"](n_layer=4, n_dim=128, input_dim=3, skips=[], mask_dim=K, mask_act="softmax")
    sd = mf.state_dict()
    for k, v in zip(m64.GRAD_KEYS, m64.params_for(K)):
        sd[k].copy_(torch.from_numpy(v))
    f.mask_field = mf
    return mf


def reference_run(f, mf, o, d, target, kind):
    """mask_map, loss, n, the gradient at the returned weight node and the ten parameter gradients from the reference's own train-mode render"""
    f.train()
    torch.manual_seed(SEED)
    _, _, _, weight, mask_map = f(T_NONKEY, o, d, white_bg=True)
    R, K = mask_map.shape
    y, ok = ml64.targets(target, R, K)
    y, okt = torch.from_numpy(y), torch.from_numpy(ok)
    n = int(ok.sum())
    if n == 0:
        loss = (mask_map * 0).sum()
    elif kind == "l2":
        loss = (((mask_map - y) ** 2) * okt[:, None]).sum() / (2 * n * K)
    else:
        loss = (torch.where(y != 0, -y * torch.log(mask_map + EPS), torch.zeros_like(mask_map)) * okt[:, None]).sum() / n
    ps = [dict(mf.named_parameters())[k] for k in m64.GRAD_KEYS]
    grads = torch.autograd.grad(loss, [weight] + ps, allow_unused=True)
    gw = torch.zeros_like(weight) if grads[0] is None else grads[0]
    f.eval()
    return (mg.npf(weight.detach()), mg.npf(mask_map.detach()), float(loss.detach()), n, mg.npf(gw.reshape(weight.shape)),
            {k: mg.npf(torch.zeros_like(p) if g is None else g) for k, p, g in zip(m64.GRAD_KEYS, ps, grads[1:])})


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    from helpers import load_meta
    fl = np.load(os.path.join(HERE, "flowloss.npz"))
    fx, nets = {}, {}
    for kind, nv in (("A", nvA), ("B", nvB)):
        f = nv.nvfi
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        field = r64.Field(sd, meta)
        # the first N_RAYS rays of tests/golden/flowloss.npz; the reference draws its own jitter for them (recorded).  A ray with a masked sample
        # within KINK_MARGIN rounding bounds of a MaskField kink (the trunk is the same for every K) or within 4 ulp of the weight threshold is
        # IGNORED in every case (label -1 / a NaN row): it contributes nothing, and the cases stay well-posed
        o, d = torch.from_numpy(fl[f"{kind}:rays_o"][:N_RAYS].copy()), torch.from_numpy(fl[f"{kind}:rays_d"][:N_RAYS].copy())
        Rn = len(o)
        torch.manual_seed(SEED)
        u = torch.rand(Rn, 1).numpy().reshape(-1)
        fx[f"{kind}:u"] = u.astype(np.float32)
        mf = attach(R, f, 8)
        weight0 = reference_run(f, mf, o, d, np.zeros(Rn, np.int32), "l2")[0]
        f.mask_field = None
        y = ml64.maskloss64(field, m64.params_for(8), o.numpy(), d.numpy(), T_NONKEY, weight0, u, np.zeros(Rn, np.int32))
        bad = np.zeros(Rn, bool)
        bad[y["idx"][y["margin"] < m64.KINK_MARGIN][:, 0]] = True
        bad |= (np.abs(weight0.astype(np.float64) - field.thres) <= 4 * float(np.spacing(np.float32(field.thres)))).any(1)
        print(f"{kind}: {int(bad.sum())} of {Rn} rays ignored in every case (a masked sample within {m64.KINK_MARGIN} rounding bounds of a kink, or 4 ulp of the threshold): {np.nonzero(bad)[0]}")
        assert (~bad).sum() >= 24
        fx[f"{kind}:ignored"] = bad
        rng = np.random.default_rng(31)
        cases = []
        for K in (8, 17):
            lab = rng.integers(0, K, Rn).astype(np.int32)
            soft = rng.random((Rn, K)).astype(np.float32)
            soft = (soft / soft.sum(1, keepdims=True) * rng.random((Rn, 1)).astype(np.float32)).astype(np.float32)
            lab[bad] = -1
            soft[bad, 0] = np.nan
            lab3 = lab.copy()
            good = np.nonzero(~bad)[0]
            lab3[good[[3, 11, 19]]] = -1
            lab3[good[5]] = K
            if K == 8:
                cases += [("c0", K, "l2", lab), ("c1", K, "ce", lab), ("c2", K, "ce", soft), ("c3", K, "ce", lab3), ("c4", K, "ce", np.full(Rn, -1, np.int32))]
            else:
                cases += [("c5", K, "ce", lab3)]
        for name, K, lk, target in cases:
            key = f"{kind}:{name}"
            mf = attach(R, f, K)
            weight, mask_map, loss, n, gw, grads = reference_run(f, mf, o, d, target, lk)
            f.mask_field = None
            a = (field, m64.params_for(K), o.numpy(), d.numpy(), T_NONKEY, weight, u, target)
            y64 = ml64.maskloss64(*a, kind=lk, eps=EPS)
            y32 = ml64.maskloss64(*a, kind=lk, eps=EPS, dtype=torch.float32, want_margin=False)
            assert np.array_equal(weight, weight0), (key, "the same seed, the same rays: the same weights")
            counted = ~bad[y64["idx"][:, 0]]
            assert y64["M"] and (y64["margin"][counted] >= m64.KINK_MARGIN).all(), (key, float(y64["margin"][counted].min()))
            assert not (np.abs(weight[~bad].astype(np.float64) - field.thres) <= 4 * float(np.spacing(np.float32(field.thres)))).any(), key
            assert n == y64["n"], key
            assert not gw[~y64["mask"]].any(), (key, "the weight node's gradient is zero outside the masked samples")
            floor = np.array(ml64.d32(y32, y64))
            got = dict(mask_map=mask_map, loss=loss, g_weights=gw, **grads)
            ref_err = ml64.d32(got, y64)
            print(f"{key}: {lk} K={K} M={y64['M']} n={n} loss={loss:.6g} floor(fp32 yardstick; mask_map, loss, g_weights, worst of the ten)={floor} "
                  f"reference-vs-yardstick={ref_err}")
            fx[key + ":kind"], fx[key + ":K"], fx[key + ":target"] = np.array(lk), np.int64(K), target
            fx[f"{kind}:weight_masked"], fx[f"{kind}:mask"] = weight[y64["mask"]], np.packbits(y64["mask"])
            assert not gw[bad].any(), key
            fx[key + ":mask_map"], fx[key + ":loss"], fx[key + ":n"] = mask_map, np.float64(loss), np.int64(n)
            fx[key + ":g_weights"] = gw[y64["mask"] & ~bad[:, None]]
            fx[key + ":M"], fx[key + ":floor"] = np.int64(y64["M"]), floor
            if name == "c4":
                assert loss == 0.0 and not gw.any() and all(not v.any() for v in grads.values()), key
                continue
            dst = nets.setdefault(f"maskloss_grads_{kind}{1 if name in ('c0', 'c1', 'c2') else 2}.npz", {})
            for k, v in grads.items():
                dst[f"{key}:{k}"] = v
    for fn, dd in nets.items():
        np.savez_compressed(os.path.join(HERE, fn), **dd)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
        assert os.path.getsize(os.path.join(HERE, fn)) < (1 << 20)
    out = os.path.join(HERE, "maskloss.npz")
    np.savez_compressed(out, **fx)
    print("wrote maskloss.npz", os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
