"""The float64 restatement of the render step (tests/render64.py) against the reference's own outputs in tests/golden/hotpath.npz, fields A and
B: this pins the yardstick that tests/test_gpu_render64.py holds the device kernels to.

Train cases (train_nonkey: one RK2 step, train_key: no warp, train_extrap: 2 steps on field A and 8 on field B with step rejection) with the stored
jitter, white coin, target and per-sample weights gw: rgb, depth, acc, weight, the loss and EVERY stored gradient tensor; goldens stored empty
(the acceleration net, and the velocity net at a keyframe) must come out absent or exactly zero.  Eval cases key, nonkey, extrap, transfer, flipbg:
the maps.  The `amask` golden (the eval render through an occupancy volume, render64's `alpha_volume`) is held in tests/test_alpha64_golden.py,
next to the rest of the occupancy path.

Measured (CPU): float64 against the fp32 goldens, worst over the cases: gradients max(maxrel, rel_l2) 3.0e-6 (A:train_nonkey density_plane_time.0;
1.2e-6 - 1.9e-6 in the other cases), loss rel err 8.4e-8, maps: no element leaves helpers.FP32_FLOOR at all (max abs err rgb 2.6e-7, acc 4.2e-7,
weight 1.0e-6, depth 1.8e-6); where |golden| > 1e-3 the worst relative error is 1.2e-6 (acc, A:render_transfer; 8.6e-7 in the train cases).  The cross-check, render64 evaluated in float32
against itself in float64 on the same cases, gives the same picture: gradients 2.8e-6 worst (the same tensor), maps within 1.0e-6 / 1.8e-6 (depth)
absolute.  So what is left is the goldens' own fp32 rounding.  Bounds = 3 x the worst measured, rounded up: 1e-5 on the gradients, rtol 4e-6 +
FP32_FLOOR on the maps, 3e-7 on the loss - fifty times under what the device is held to against the same goldens (5e-4 / 1e-4).

Mask flips of the reference alone: on every golden case the appearance mask of the float32 evaluation equals the float64 one (0 differing samples
of 6 860 - 8 245 masked ones); the condition asserted is <= 0.05 % of the masked samples, each within 1e-6 of the threshold."""
import numpy as np
import pytest
import torch

import render64 as r64
from conftest import maxrel, rel_l2
from helpers import FP32_FLOOR, load_meta

KINDS = ["A", "B"]
GRAD_BOUND = 1e-5
MAP_RTOL = 4e-6
LOSS_RTOL = 3e-7


@pytest.fixture(scope="module")
def fields64():
    ma, sa = load_meta("A")
    mb, sb = load_meta("B")
    for k, v in sa.items():      # field B shares the MLPs of field A
        sb.setdefault(k, v)
    return {"A": (r64.Field(sa, ma), ma), "B": (r64.Field(sb, mb), mb)}


def _maps(r, gold, pre, label):
    for m in ("rgb", "depth", "acc", "weight"):
        ref = gold[pre + m].astype(np.float64)
        err = np.abs(r[m] - ref)
        big = np.abs(ref) > 1e-3
        print(f"[render64] {label}:{m}: max abs err {err.max():.2e}, max rel err where |ref| > 1e-3 {(err[big] / np.abs(ref[big])).max():.2e}")
        assert (err <= MAP_RTOL * np.abs(ref) + FP32_FLOOR[m]).all(), (label, m, float(err.max()))


def _mask_condition(r, r32, thres, label):
    diff = r["app_mask"] != r32["app_mask"]
    n, masked = int(diff.sum()), int(r["app_mask"].sum())
    dist = np.abs(r["weight"][diff] - thres)
    print(f"[render64] {label}: float32 / float64 masks differ on {n} of {masked} masked samples" + (f", max |w - thres| {dist.max():.2e}" if n else ""))
    assert n <= 5e-4 * masked, (label, n, masked)
    assert (dist <= 1e-6).all(), (label, float(dist.max()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["train_nonkey", "train_key", "train_extrap"])
def test_render64_matches_the_reference_train_goldens(gold, fields64, kind, name):
    f, meta = fields64[kind]
    pre = f"{kind}:{name}:"
    o, d = gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"]
    wb = bool(meta["white_background"]) or bool(gold[pre + "coin"])
    loss = r64.Loss(gold[pre + "target"], 0.01, 0.02, gold[pre + "gw"])
    t = float(np.float32(gold[pre + "t"]))
    r = r64.render64(f, o, d, t, gold[pre + "u"], wb, loss=loss)
    r32 = r64.render64(f, o, d, t, gold[pre + "u"], wb, loss=loss, dtype=torch.float32)
    nsteps = len(r["plan"]["steps"])
    assert nsteps == {"train_nonkey": 1, "train_key": 0, "train_extrap": 2 if kind == "A" else 8}[name], nsteps
    assert r["app_mask"].sum() > 5000 and (r["flips"].size == 0)
    _mask_condition(r, r32, f.thres, pre)
    _maps(r, gold, pre, pre)
    for m in ("rgb", "depth", "acc", "weight"):
        print(f"[render64] {pre}{m}: float32 evaluation against float64 max abs {np.abs(r32[m] - r[m]).max():.2e}")
    lerr = abs(r["loss"] - float(gold[pre + "loss"][0])) / abs(float(gold[pre + "loss"][0]))
    checked, worst, worst32 = 0, (0.0, None), (0.0, None)
    bad = []
    gp = pre + "grad:nvfi."
    for k in gold.files:
        if not k.startswith(gp) or k == gp + "basis_mat_density.weight":
            continue
        pn, ref = k[len(gp):], gold[k]
        got = r["grads"].get(pn)
        if ref.size == 0:
            assert got is None or not np.any(got), pn
            continue
        e = max(maxrel(got, ref), rel_l2(got, ref))
        worst = max(worst, (e, pn))
        worst32 = max(worst32, (max(maxrel(r32["grads"][pn], got), rel_l2(r32["grads"][pn], got)), pn))
        if not e <= GRAD_BOUND:
            bad.append((pn, e))
        checked += 1
    print(f"[render64] {pre} loss rel err {lerr:.2e}; {checked} gradient tensors, worst against the golden {worst[0]:.2e} ({worst[1]}), "
          f"float32 evaluation against float64 {worst32[0]:.2e} ({worst32[1]})")
    assert lerr <= LOSS_RTOL, lerr
    assert not bad, bad
    assert checked >= (31 if (kind, name) == ("A", "train_nonkey") else 5), checked


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["key", "nonkey", "extrap", "transfer", "flipbg"])
def test_render64_matches_the_reference_eval_goldens(gold, fields64, kind, name):
    f, meta = fields64[kind]
    pre = f"{kind}:render_{name}:"
    o, d = gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"]
    wb = bool(meta["white_background"]) != (name == "flipbg")
    t = float(np.float32(gold[f"{kind}:render_nonkey:t" if name == "flipbg" else pre + "t"]))
    kw = dict(loss=None, grads=False, transfer=(name == "transfer"))
    r = r64.render64(f, o, d, t, None, wb, **kw)
    r32 = r64.render64(f, o, d, t, None, wb, dtype=torch.float32, **kw)
    _mask_condition(r, r32, f.thres, pre)
    _maps(r, gold, pre, pre)


def test_render64_sums_over_rays_and_cuts(gold, fields64):
    """the pieces the GPU file's bookkeeping relies on: a subset of the rays rendered on its own gives those rays' maps and loss terms; another
    appearance mask through with_mask equals a full recomputation under it; detach() of a sample changes only that sample's branch"""
    f, meta = fields64["A"]
    pre = "A:train_nonkey:"
    o, d, u = gold["A:rays_o"], gold["A:rays_d"], gold[pre + "u"]
    loss = r64.Loss(gold[pre + "target"], 0.01, 0.02, gold[pre + "gw"])
    t = float(np.float32(gold[pre + "t"]))
    full = r64.render64(f, o, d, t, u, True, loss=loss, chunk=100)
    sub = np.array([3, 17, 100, 255])
    part = r64.render64(f, o, d, t, u, True, loss=loss, rays=sub)
    np.testing.assert_allclose(part["rgb"], full["rgb"][sub], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(part["loss_rays"], full["loss_rays"][sub], rtol=1e-12)
    mask = full["app_mask"].copy()
    ij = r64.list_order(mask)
    for k in (5, len(ij) // 2, len(ij) - 1):      # drop three masked samples of three different rays
        mask[ij[k][0], ij[k][1]] = False
    upd = r64.with_mask(full, mask)
    again = r64.render64(f, o, d, t, u, True, loss=loss, app_mask=mask)
    assert len(upd["flips"]) == 3 and abs(upd["loss"] - again["loss"]) <= 1e-12 * abs(again["loss"])
    for n in r64.NAMES:
        np.testing.assert_allclose(upd["grads"][n], again["grads"][n], rtol=1e-8, atol=1e-12 * np.abs(again["grads"][n]).max())
    last = ij[-1:]
    cut = r64.detach(full, last, "rgb")
    moved = {n: max(maxrel(cut[n], full["grads"][n]), rel_l2(cut[n], full["grads"][n])) for n in r64.NAMES}
    assert max(moved[n] for n in r64.MLP_NAMES) > 0 and max(moved[n] for n in r64.NAMES if n.startswith("density")) < 1e-12, moved
    cut = r64.detach(full, np.argwhere(full["valid"])[-1:], "sigma")
    assert maxrel(cut["density_plane_space.0"], full["grads"]["density_plane_space.0"]) > 0


# ---------------------------------------------------------------------------------------------------------------- field D: SH shading
# tests/golden/r2.npz, field D = field A's geometry with shadingMode "SH" (make_golden_r2.py): two eval renders (rgb, depth, acc; no weight map
# is stored) and one train render at t = 19/60 with the loss mse + 0.01 mean(depth) and its 25 gradient tensors.  Same rules and bounds as A and B.
# Measured (CPU): float64 against the fp32 goldens: gradients 1.8e-6 worst (density_plane_time.2), loss rel err 3.8e-8, maps max abs err rgb 2.6e-7,
# acc 4.7e-7, depth 2.2e-6.  render64 in float32 against itself in float64 on D:train, per family (the floor of the SH bounds of
# tests/test_gpu_render64.py; asserted to fit three times under GRAD_BOUND): density 1.9e-6, app 1.1e-6, mlp (basis_mat) 3.4e-7, vel 2.7e-7; the
# masks agree on all 7 067 - 7 104 masked samples.  The wrong variant (basis 6 with zz - xx - yy) moves rgb by 2.9e-2 and takes all 25 gradient
# tensors out of the bound (basis_mat.weight by 2.3e-1).  No masked colour of D:train lies within 4 x its rounding bound of a kink (relu_margin).
@pytest.fixture(scope="module")
def field_d():
    import os
    from conftest import GOLD
    g2 = np.load(os.path.join(GOLD, "r2.npz"))
    meta, _ = load_meta("A")
    sd = {k[len("D:sd:"):]: g2[k] for k in g2.files if k.startswith("D:sd:")}
    f = r64.Field(sd, meta)
    assert f.sh and f.names == r64.SH_NAMES and not any(n in f.p32 for n in r64.MLP_NAMES)
    return f, g2


def _maps_d(r, g2, pre, label):
    for m in ("rgb", "depth", "acc"):
        if pre + m not in g2.files:
            continue
        ref = g2[pre + m].astype(np.float64)
        err = np.abs(r[m] - ref)
        print(f"[render64] {label}:{m}: max abs err {err.max():.2e}")
        assert (err <= MAP_RTOL * np.abs(ref) + FP32_FLOOR[m]).all(), (label, m, float(err.max()))


@pytest.mark.parametrize("name,t", [("nonkey", 19.0 / 60.0), ("key", 0.25)])
def test_render64_sh_matches_the_reference_eval_goldens(gold, field_d, name, t):
    f, g2 = field_d
    o, d = gold["A:rays_o"], gold["A:rays_d"]
    kw = dict(loss=None, grads=False)
    r = r64.render64(f, o, d, t, None, True, **kw)
    r32 = r64.render64(f, o, d, t, None, True, dtype=torch.float32, **kw)
    assert len(r["plan"]["steps"]) == (1 if name == "nonkey" else 0)
    _mask_condition(r, r32, f.thres, f"D:render_{name}:")
    _maps_d(r, g2, f"D:render_{name}:", f"D:render_{name}")
    bad = r64.render64(f, o, d, t, None, True, wrong=True, **kw)
    err = np.abs(bad["rgb"] - g2[f"D:render_{name}:rgb"])
    print(f"[render64] D:render_{name}: the wrong basis moves rgb by {err.max():.2e}")
    assert (err > MAP_RTOL * np.abs(g2[f"D:render_{name}:rgb"]) + FP32_FLOOR["rgb"]).any()


def test_render64_sh_matches_the_reference_train_golden(gold, field_d):
    f, g2 = field_d
    o, d = gold["A:rays_o"], gold["A:rays_d"]
    loss = r64.Loss(g2["D:train:target"], 0.01)          # make_golden_r2.py: mse + 0.01 mean(depth)
    kw = dict(loss=loss)
    r = r64.render64(f, o, d, 19.0 / 60.0, g2["D:train:u"], True, **kw)
    r32 = r64.render64(f, o, d, 19.0 / 60.0, g2["D:train:u"], True, dtype=torch.float32, **kw)
    bad = r64.render64(f, o, d, 19.0 / 60.0, g2["D:train:u"], True, wrong=True, **kw)
    assert len(r["plan"]["steps"]) == 1 and r["app_mask"].sum() > 5000 and r["flips"].size == 0
    assert set(r["grads"]) == set(r64.SH_NAMES)
    _mask_condition(r, r32, f.thres, "D:train:")
    _maps_d(r, g2, "D:train:", "D:train")
    for m in ("rgb", "depth", "acc", "weight"):
        print(f"[render64] D:train:{m}: float32 evaluation against float64 max abs {np.abs(r32[m] - r[m]).max():.2e}")
    gl = float(g2["D:train:loss"].reshape(-1)[0])
    lerr = abs(r["loss"] - gl) / abs(gl)
    gp = "D:train:grad:nvfi."
    checked, worst, fam32, seen, out = 0, (0.0, None), {}, [], []
    for k in g2.files:
        if not k.startswith(gp):
            continue
        pn, ref = k[len(gp):], g2[k]
        got = r["grads"][pn]
        e = max(maxrel(got, ref), rel_l2(got, ref))
        worst = max(worst, (e, pn))
        fm = r64.FAMILY[pn]
        fam32[fm] = max(fam32.get(fm, 0.0), max(maxrel(r32["grads"][pn], got), rel_l2(r32["grads"][pn], got)))
        if max(maxrel(bad["grads"][pn], ref), rel_l2(bad["grads"][pn], ref)) > GRAD_BOUND:
            seen.append(pn)
        if not e <= GRAD_BOUND:
            out.append((pn, e))
        checked += 1
    print(f"[render64] D:train: loss rel err {lerr:.2e}; {checked} gradient tensors, worst against the golden {worst[0]:.2e} ({worst[1]}); float32 "
          "evaluation against float64 per family " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(fam32.items()))
          + f"; the wrong basis leaves the bound on {len(seen)} tensors (basis_mat.weight "
          f"{max(maxrel(bad['grads']['basis_mat.weight'], g2[gp + 'basis_mat.weight']), rel_l2(bad['grads']['basis_mat.weight'], g2[gp + 'basis_mat.weight'])):.2e}), "
          f"rgb by {np.abs(bad['rgb'] - g2['D:train:rgb']).max():.2e}")
    assert lerr <= LOSS_RTOL, lerr
    assert not out, out
    assert checked == 25, checked
    assert all(3 * v <= GRAD_BOUND for v in fam32.values()), fam32
    # the wrong variant is seen: on the map and on basis_mat and the appearance planes
    err = np.abs(bad["rgb"] - g2["D:train:rgb"])
    assert (err > MAP_RTOL * np.abs(g2["D:train:rgb"]) + FP32_FLOOR["rgb"]).any()
    assert "basis_mat.weight" in seen and any(n.startswith("app_plane") for n in seen), seen


def test_render64_sh_bookkeeping(gold, field_d):
    """with_mask and detach on an SH field (no render-MLP names anywhere), and relu_margin's SH form: finite exactly on the masked samples"""
    f, g2 = field_d
    o, d, u = gold["A:rays_o"], gold["A:rays_d"], g2["D:train:u"]
    loss = r64.Loss(g2["D:train:target"], 0.01)
    full = r64.render64(f, o, d, 19.0 / 60.0, u, True, loss=loss)
    mask = full["app_mask"].copy()
    ij = r64.list_order(mask)
    mask[ij[7][0], ij[7][1]] = False
    upd = r64.with_mask(full, mask)
    again = r64.render64(f, o, d, 19.0 / 60.0, u, True, loss=loss, app_mask=mask)
    for n in f.names:
        np.testing.assert_allclose(upd["grads"][n], again["grads"][n], rtol=1e-8, atol=1e-12 * np.abs(again["grads"][n]).max())
    cut = r64.detach(full, ij[-1:], "rgb")
    moved = {n: maxrel(cut[n], full["grads"][n]) for n in f.names}
    assert moved["basis_mat.weight"] > 0 and max(moved[n] for n in f.names if n.startswith("density")) < 1e-12, moved
    ms, mr = r64.relu_margin(f, o, d, 19.0 / 60.0, u)
    assert ms.shape == full["app_mask"].shape + (3,) and mr.shape == (o.shape[0], 3)
    assert (np.isfinite(ms).all(-1) == full["app_mask"]).all() and (ms[full["app_mask"]] > 0).all()
    print(f"[render64] D:train: masked (sample, channel) colours within 4 x their rounding bound of the ReLU kink: {int((ms < 4).sum())} of "
          f"{3 * int(full['app_mask'].sum())}; (ray, channel) within 4 x of a clamp kink: {int((mr < 4).sum())} of {mr.size}")
