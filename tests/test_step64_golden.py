"""The yardstick of one training iteration (tests/step64.py) against the reference's own loop: tests/golden/r2.npz holds, under A:loop:*, three
iterations of train_nvfi.py:139-249 (--static_dynamic) that tests/golden/make_golden_r2.py ran with the reference on field A in fp32 - targets, the
jitter of both renders, the collocation points and times, the total loss and loss_vel of every iteration, every parameter after the third step.
step64.free_run starts from field_A.npz and runs free in float64: iterations 2 and 3 render the field that its own gradients and Adam steps made,
and the PDE term's kept set is decided by step64.kept64 (point64.integrate64, point64.density64, alpha >= alphaMask_thres on the fp32 value).

Bounds - measured, not typed in.  Every one is 4 x the distance of the float32 run of the same yardstick from its float64 run on this case, and never
under optim64.ulp_floor (4 fp32 spacings of the quantity: the goldens are STORED in fp32):
  loss, loss_vel per iteration: optim64.bound(float32 run, float64 run);
  parameters, on the distance moved over the three steps: |dp - dp64| <= B_p x (lr_1 + lr_2 + lr_3), B_p = 4 x the largest such distance of the
  float32 run over all non-exempt elements, in units of the summed learning rate, and never under 4 spacings of the tensor's peak in those units.
  Exempt is an element whose |g64| is under B[family] x max|g64| of its tensor in any iteration (Adam divides by the gradient's own history: such an
  element may take either sign at full step length), B[family] = 3 x the largest max(maxrel, rel_l2) of the float32 run's gradients from the
  float64 run's in that family; an exempt element stays within sum_t lr_t x 1.001 / (1 - b1).  At most 2 % of a tensor of 64 or more elements may be
  exempt (a condition, asserted).  An element whose gradient is exactly zero in all three iterations does not move at all.

Measured (CPU, 15 s): float32 run / golden, relative distance from the float64 run
  loss       it 0: 5.5e-9 / 8.3e-8   it 1: 7.6e-9 / 1.0e-7   it 2: 5.8e-9 / 1.4e-8      bound 2.7e-7 - 3.2e-7 (the fp32 spacing floor)
  loss_vel   it 0: 3.4e-8 / 1.4e-8   it 1: 8.4e-8 / 1.2e-7   it 2: 4.9e-9 / 1.3e-7      bound 3.1e-7 - 3.4e-7 (floor; it 1: 3.4e-7 = 4 x 8.4e-8)
  the kept sets hold 1125 / 1146 / 1164 of 4096 points; the nearest decision is 4e-9 from the threshold in alpha, inside the 6e-8 grid on which an
  fp32 `1 - exp(-x)` sits there - the decision has to be taken on the fp32 value as the reference takes it (with the float64 alpha point 1146 of
  iteration 1 falls out and loss_vel moves by 2.1e-4).
  gradients, 3 x (float32 run against float64 run), worst of the three iterations: density 2.9e-5, app 8.3e-6, mlp 1.4e-6, vel 1.9e-6;
  parameters, in units of the summed learning rate: float32 run 1.6e-4 (renderModule.mlp.0.weight), golden 9.5e-5 (renderModule.mlp.2.weight),
  B_p 6.5e-4; the exempt share of an iteration is at most 1.8 % outside OVER_CAP (below): the 2 % cap is NOT met by the four tensors listed there.
Wrong variants of the yardstick on this case, each run free in float64 (what they move, against the bound):
  (a) weights decayed after use: the total loss of iteration 0 by 8.5e-6 (bound 2.7e-7), parameters by 1.3e-2 (B_p 6.5e-4) - SEEN;
  (b) learning rate decayed before the step: loss_vel of iteration 2 by 6.8e-5 (bound 3.4e-7), parameters by 2.6e-2 - SEEN;
  (c) bias corrections at t - 1 (from iteration 1 on): loss of iteration 2 by 8.8e-3, parameters by 0.65 - SEEN.
The list BLIND below names what cannot be seen here; the test asserts that it is blind, so that the entry cannot outlive its reason."""
import os

import numpy as np
import pytest
import torch

import optim64
import step64 as s64
from conftest import GOLD, maxrel, rel_l2
from helpers import load_meta

BLIND = set()                 # (variant, observable) pairs that this case cannot see: none - every variant leaves loss, loss_vel and parameters
EXEMPT_CAP = 0.02
# Tensors of the golden case that cannot keep the cap (the case is what the reference recorded), each with a ceiling just above its measured share:
# the appearance time planes - both renders have their base keyframe at row 1 of 4, whose fp32 row coordinate lies 6e-8 beside the integer, so a
# second row gets a weight of that size and, with no regulariser on these planes, a gradient of 1e-7 of the peak: a quarter of the tensor (measured
# 25.68 %, 25.93 %, 25.34 %) - and density_plane_space.2, 2.23 % of whose texels see less than 2.9e-5 of the peak.  A tensor that is not listed keeps
# the 2 %; a listed one keeps its ceiling and has to be over the cap, or the entry has outlived its reason.
OVER_CAP = {"app_plane_time.0": 0.260, "app_plane_time.1": 0.262, "app_plane_time.2": 0.256, "density_plane_space.2": 0.025}


def _inputs(g2, gold, meta):
    o, d = gold["A:rays_o"], gold["A:rays_d"]
    ts = float(meta["tmax"]) / (int(meta["num_keyframes"]) - 1)
    out = []
    for it in range(3):
        b = [dict(o=o, d=d, target=g2["A:loop:target1"], u=g2[f"A:loop:{it}:u1"], t=19.0 / 60.0),
             dict(o=o, d=d, target=g2["A:loop:target2"], u=g2[f"A:loop:{it}:u2"], t=ts)]
        out.append(dict(batches=b, points=g2[f"A:loop:{it}:points"], t=g2[f"A:loop:{it}:t"]))
    return out


@pytest.fixture(scope="module")
def runs():
    g2, gold = np.load(os.path.join(GOLD, "r2.npz")), np.load(os.path.join(GOLD, "hotpath.npz"))
    meta, sd = load_meta("A")
    out = {}
    for key, dt, var in (("f64", torch.float64, None), ("f32", torch.float32, None), ("a", torch.float64, "a"), ("b", torch.float64, "b"),
                         ("c", torch.float64, "c")):
        f, p = s64.make_field(sd, meta)
        out[key] = s64.free_run(f, p, _inputs(g2, gold, meta), dtype=dt, variant=var)
    out["start"] = s64.make_field(sd, meta)[1]
    out["gold"] = g2
    return out


def _metric(a, b):
    return max(maxrel(a, b), rel_l2(a, b))


def _lr_sum(name):
    return sum(s64.schedule(it)["lr_plane" if "plane" in name else "lr_net"] for it in range(3))


def _derive(runs):
    """the bounds, from the float32 and float64 runs alone"""
    r64_, r32 = runs["f64"], runs["f32"]
    start = runs["start"]
    B = dict.fromkeys(s64.FAMILIES, 0.0)
    for a, b in zip(r32, r64_):
        for n in s64.NAMES:
            if np.abs(b["grads"][n]).max() > 0:
                B[s64.FAMILY[n]] = max(B[s64.FAMILY[n]], 3.0 * _metric(a["grads"][n], b["grads"][n]))
    exempt, zero, share = {}, {}, {}
    for n in start:
        gs = [o["grads"][n] for o in r64_]
        fam = s64.FAMILY.get(n)
        exempt[n] = np.zeros(start[n].shape, bool)
        share[n] = 0.0
        for g in gs:
            if fam is not None and np.abs(g).max() > 0:
                ex = (np.abs(g) < B[fam] * np.abs(g).max()) & (g != 0)
                share[n] = max(share[n], float(ex.mean()))
                exempt[n] |= ex
        zero[n] = np.all([g == 0 for g in gs], axis=0)
    Bp, floor = 0.0, {}
    for n in start:
        d32 = np.asarray(r32[-1]["p"][n], np.float64) - start[n]
        d64 = r64_[-1]["p"][n] - start[n]
        e = np.abs(d32 - d64)[~exempt[n]] / _lr_sum(n)
        floor[n] = 4.0 * float(np.spacing(np.float32(np.abs(start[n]).max()))) / _lr_sum(n)
        if e.size:
            Bp = max(Bp, 4.0 * float(e.max()))
    vb = {("loss", it): optim64.bound(r32[it]["loss"], r64_[it]["loss"]) for it in range(3)}
    vb.update({("lv", it): optim64.bound(r32[it]["lv"], r64_[it]["lv"]) for it in range(3)})
    return dict(B=B, Bp=Bp, floor=floor, exempt=exempt, zero=zero, value=vb, share=share)


def _violations(outs, runs, D, ref=None):
    """the observables of a free run `outs` held against `ref` (default: the goldens): list of (observable, figure, bound)"""
    g2, start, r64_ = runs["gold"], runs["start"], runs["f64"]
    bad, fig = [], {}
    for it in range(3):
        for key, gk in (("loss", "loss"), ("lv", "loss_vel")):
            want = float(g2[f"A:loop:{it}:{gk}"].reshape(-1)[0]) if ref is None else ref[it][key]
            e = abs(outs[it][key] - want) / abs(want)
            fig[(key, it)] = e
            if e > D["value"][(key, it)]:
                bad.append(((key, it), e, D["value"][(key, it)]))
    worst = (0.0, "")
    for n in start:
        want = g2["A:loop:final:nvfi." + n].astype(np.float64) if ref is None else np.asarray(ref[-1]["p"][n], np.float64)
        dp, dw = np.asarray(outs[-1]["p"][n], np.float64) - start[n], want - start[n]
        err = np.abs(dp - dw) / _lr_sum(n)
        ex = D["exempt"][n]
        b = max(D["Bp"], D["floor"][n])
        e = float(err[~ex].max()) if (~ex).any() else 0.0
        worst = max(worst, (e, n))
        if e > b:
            bad.append((("p", n), e, b))
        if ex.any() and float(err[ex].max()) > 1.001 / (1 - s64.B1):
            bad.append((("p exempt", n), float(err[ex].max()), 1.001 / (1 - s64.B1)))
        if ref is None and D["zero"][n].any() and np.any(want[D["zero"][n]] != start[n][D["zero"][n]]):
            bad.append((("p zero-gradient", n), 0.0, 0.0))
    fig["p"] = worst
    return bad, fig


def test_step64_follows_the_reference_loop(runs):
    D = _derive(runs)
    r64_, r32 = runs["f64"], runs["f32"]
    print("[step64 golden] kept", [o["n_kept"] for o in r64_], "nearest kept decision", [f"{o['kept_margin']:.1e}" for o in r64_])
    print("[step64 golden] B[family] = 3 x float32 gradient figure:", {k: f"{v:.2e}" for k, v in D["B"].items()}, "B_p", f"{D['Bp']:.2e}")
    print("[step64 golden] largest exempt share of an iteration, per tensor (only those with any):",
          {k: f"{v:.2%}" for k, v in D["share"].items() if v > 0})
    _, f32 = _violations(r32, runs, D, ref=r64_)
    bad, fg = _violations(r64_, runs, D)
    for k in sorted(D["value"]):
        print(f"[step64 golden] {k}: float32 run {f32[k]:.2e}, golden {fg[k]:.2e}, bound {D['value'][k]:.2e}")
    print(f"[step64 golden] parameters (units of the summed lr): float32 run {f32['p'][0]:.2e} ({f32['p'][1]}), golden {fg['p'][0]:.2e} ({fg['p'][1]}), "
          f"B_p {D['Bp']:.2e}, spacing floors {min(D['floor'].values()):.1e} - {max(D['floor'].values()):.1e}")
    assert [o["n_kept"] for o in r64_] == [o["n_kept"] for o in r32], "the float32 and float64 runs keep different points"
    for n, sh in D["share"].items():
        if runs["start"][n].size >= 64:
            assert sh <= OVER_CAP.get(n, EXEMPT_CAP), (n, "exempt share", sh)
    for n in OVER_CAP:
        assert D["share"][n] > EXEMPT_CAP, (n, "is listed in OVER_CAP but keeps the cap", D["share"][n])
    assert not bad, bad
    assert r64_[2]["loss"] < r64_[1]["loss"] < r64_[0]["loss"]


@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_the_bounds_see_the_wrong_variant(runs, variant):
    """each wrong variant, run free in float64, has to leave a bound that the right run keeps - or be listed as BLIND for that observable"""
    D = _derive(runs)
    bad, fig = _violations(runs[variant], runs, D)
    kinds = {("loss" if k[0] == "loss" else "loss_vel" if k[0] == "lv" else "parameters") for k, _, _ in bad}
    print(f"[step64 golden] variant {variant}: leaves {sorted(kinds)}; worst figures "
          + ", ".join(f"{k}: {e:.2e} (bound {b:.2e})" for k, e, b in sorted(bad, key=lambda x: -x[1] / max(x[2], 1e-300))[:4]))
    for obs in ("loss", "loss_vel", "parameters"):
        if (variant, obs) in BLIND:
            assert obs not in kinds, (variant, obs, "is listed as blind but is seen")
    assert kinds, (variant, "no observable of the golden case sees it", {k: v for k, v in fig.items() if k != "p"}, fig["p"])
