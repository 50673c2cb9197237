"""The float64 restatement of the stand-alone point queries (tests/point64.py) against the reference's own outputs that are already under
tests/golden/hotpath.npz: this pins the yardstick that tests/test_gpu_point64.py holds the device to.  No fixture is added.

  {A,B}:vel:u / vel:gated                 vel64 on 257 points of [-1.05, 1.05]^3 x [0, 1]; the zero pattern of the gated output is exact
  {A,B}:integrate:xk / integrate_fwd:xk   integrate64 with per-point times: t in [0, 1) against its snapped keyframe (0 - 2 steps on A, 0 - 10 on B,
                                          both signs, extrapolation beyond tmax), and t = 0 towards [0.5, 0.75) (5 - 6 steps on A, 21 - 30 on B)
  {A,B}:feat:density / feat:sigma / feat:app, {A,B}:mlp:rgb, sh:rgb

Bound of each golden: |float64 yardstick - golden| <= rtol |golden| + atol with (rtol, atol) = point64.bound of the float32 evaluation of the
yardstick against its float64 evaluation on the same inputs (alpha64.floors: abs over |ref| <= 1e-2, rel over the rest; x 3; never under one fp32
ulp of the tensor's scale).  Measured (CPU, torch 2.10): the float32 evaluation reproduces every golden to within 1.5e-8 absolute / 5e-7 relative
(most bit for bit), so what the bound holds is fp32 rounding in the golden itself; float64 against the golden, abs / rel:
  vel:u 5.7e-8 / 6.8e-7 (A), 6.7e-8 / 3.9e-7 (B)     integrate 7.6e-9 / 7.6e-8, 2.4e-9 / 2.9e-7      integrate_fwd 1.6e-8 / 5.3e-7, 4.6e-8 / 3.1e-7
  density 1.2e-7 / 6.5e-6, 1.0e-7 / 6.8e-6           sigma 1.8e-8 / 3.1e-6, 1.5e-8 / 1.9e-8          app features 1.3e-8, 1.0e-8 (all under 1e-2)
  mlp:rgb 0 / 1.2e-7, 0 / 1.2e-7                     sh 1.1e-8 / 3.2e-6
Each deliberately wrong variant of point64 lands outside the bound of its golden, by (abs / rel as floors gives them): integrate 8e-2 / 1.8 (A),
5e-4 / 4.7 (B); vel 0.5 / 0.9; density 6 / 6; mlp 2.7e-2 rel; sh 0.24 / 0.77.

The cases of the GPU file: the float32 floor of every (call, field, case) is measured again here - for vel, vel_gated and integrate in both plain fp32
orders, torch's blocked sums and the term-by-term sum of point64._linear_chain - and 3 x it must stay inside the bound of point64.FLOOR's entry; the points within 4 fp32 ulp of a gate face are at most 0.5 % of a case (the nine points that test_vel_eval places ON the gate box are
counted apart: their decision compares equal numbers); field B's `mixed` case rejects steps; the uniform schedule equals advect64.schedule."""
import os

import numpy as np
import pytest
import torch

import advect64
import alpha64 as a64
import point64 as p64
from conftest import GOLD
from helpers import load_meta


@pytest.fixture(scope="module")
def pfields():
    return cpu_fields()


def cpu_fields():
    ma, sa = load_meta("A")
    mb, sb = load_meta("B")
    for k, v in sa.items():      # field B shares the MLPs of field A
        sb.setdefault(k, v)
    g2 = np.load(os.path.join(GOLD, "r2.npz"))
    sd = {k[5:]: g2[k] for k in g2.files if k.startswith("D:sd:")}
    return {"A": p64.field_of(sa, ma), "B": p64.field_of(sb, mb), "D": p64.field_of(sd, dict(ma, aabb=sd["nvfi.aabb"]), sh=True)}


def _pair(fn, *a, **kw):
    return fn(*a, dtype=torch.float64, **kw), fn(*a, dtype=torch.float32, **kw)


def _hold(label, y64, y32, ref, wrong):
    """float64 yardstick against the golden `ref` under the bound of its float32 evaluation; the wrong variant outside it.  Returns whether the
    wrong variant is seen."""
    ref = np.asarray(ref, np.float64).reshape(np.asarray(y64).shape)
    fa, fr = a64.floors(y32, y64)
    ga, gr = a64.floors(ref, y64)
    rtol, atol = p64.bound(fa, fr, float(np.abs(ref).max()))
    e = p64.excess(y64, ref, rtol, atol)
    ew = None if wrong is None else p64.excess(wrong, ref, rtol, atol)
    print(f"[point64] {label}: float64 against the golden abs {ga:.2e} rel {gr:.2e}; float32 evaluation against float64 abs {fa:.2e} rel {fr:.2e}; "
          f"bound rtol {rtol:.2e} atol {atol:.2e}, excess {e:.1e}" + ("" if ew is None else f"; the wrong variant exceeds it by {ew:.1e}"))
    assert e <= 0, (label, ga, gr, fa, fr)
    return ew is not None and ew > 0


@pytest.mark.parametrize("kind", ["A", "B"])
def test_yardstick_matches_the_reference_goldens(gold, pfields, kind):
    f = pfields[kind]
    g = lambda n: gold[f"{kind}:{n}"]
    seen = {}
    # ---- VelBasis, gated and not
    y, y32 = _pair(p64.vel64, f, g("vel:xt"), False)
    seen["vel"] = _hold(f"{kind}:vel:u", y["u"], y32["u"], g("vel:u"), p64.vel64(f, g("vel:xt"), False, wrong=True)["u"])
    y, y32 = _pair(p64.vel64, f, g("vel:xt"), True)
    _hold(f"{kind}:vel:gated", y["u"], y32["u"], g("vel:gated"), None)
    assert np.array_equal(y["u"] == 0, g("vel:gated") == 0) and np.array_equal(y32["u"] == 0, g("vel:gated") == 0), "the zero pattern is exact"
    assert (~y["inside"]).sum() > 10 and y["inside"].sum() > 100
    # ---- integrate_pos with per-point times
    x0 = g("integrate:x0")
    calls = {"integrate": (g("integrate:t"), g("integrate:base")), "integrate_fwd": (np.zeros(len(x0), np.float32), g("integrate_fwd:t_target"))}
    s = []
    for name, (t, base) in calls.items():
        y, y32 = _pair(p64.integrate64, f, x0, t, base)
        w = p64.integrate64(f, x0, t, base, wrong=True)
        assert not (y["edge"] | y32["edge"]).any() and np.array_equal(y["steps"], y32["steps"])
        print(f"[point64] {kind}:{name}: steps per point {np.bincount(y['steps']).tolist()}, {y['n_rejected']} rejected")
        s.append(_hold(f"{kind}:{name}:xk", y["xk"], y32["xk"], g(name + ":xk"), w["xk"]))
        if name == "integrate":
            sg = np.sign(np.asarray(t).ravel() - np.asarray(base).ravel())
            assert (sg > 0).any() and (sg < 0).any() and (np.asarray(t) > f.tmax).any() and y["steps"].max() >= (2 if kind == "A" else 8)
    seen["integrate"] = any(s)
    assert (kind == "B") == (y["n_rejected"] > 0)
    # ---- features and density
    xyzt = g("feat:xyzt")
    y, y32 = _pair(p64.density64, f, xyzt)
    w = p64.density64(f, xyzt, wrong=True)
    s = [_hold(f"{kind}:feat:density", y["feat"], y32["feat"], g("feat:density"), w["feat"]),
         _hold(f"{kind}:feat:sigma", y["sigma"], y32["sigma"], g("feat:sigma"), w["sigma"])]
    seen["density"] = any(s)
    view = g("mlp:view")
    y, y32 = _pair(p64.app64, f, xyzt, view)
    _hold(f"{kind}:feat:app", y["feat"], y32["feat"], g("feat:app"), None)
    # ---- the render module on given features
    a = (f, g("mlp:pts"), view, g("mlp:feat"))
    y, y32 = _pair(p64.mlp64, *a)
    seen["mlp"] = _hold(f"{kind}:mlp:rgb", y, y32, g("mlp:rgb"), p64.mlp64(*a, wrong=True))
    assert all(seen.values()), ("a bound cannot see its own wrong variant", seen)


def test_sh64_matches_the_reference_golden(gold):
    y, y32 = _pair(p64.sh64, gold["sh:view"], gold["sh:feat"])
    assert _hold("sh:rgb", y, y32, gold["sh:rgb"], p64.sh64(gold["sh:view"], gold["sh:feat"], wrong=True))
    assert (gold["sh:rgb"] == 0).any() and (gold["sh:rgb"] > 0).any(), "both sides of the relu"


@pytest.mark.parametrize("kind", ["A", "B"])
def test_uniform_times_give_the_schedule_of_advect64(pfields, kind):
    f = pfields[kind]
    x = p64.case_points(f, 3, "pos")
    for t, base in ((0.93, 0.75), (19.0 / 60.0, 0.25), (0.0, 0.6), (a64.near_key_time(f), f.tmax / (f.K - 1)), (0.5, 0.5)):
        t32, b32 = np.float32(t), np.float32(base)
        r = p64.integrate64(f, x, np.full(3, t32), np.full(3, b32))
        mine = [(float(tc[0]), float(d[0]), float(tm[0])) for tc, d, tm, _ in r["trace"]]
        assert mine == advect64.schedule(f, float(t32), float(b32)), (kind, t, base)
        assert (r["steps"] == len(mine)).all()


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU file
def gpu_case_floors(fields, kind, device="cpu", sizes=None):
    """{(call, kind, case): (abs, rel)}: the float32 floor of every case of tests/test_gpu_point64.py on one field, worst over the sizes, with the
    yardstick-only conditions asserted on the way"""
    f = fields[kind]
    out = {}

    def put(key, y32, y64, keep=None):
        k = slice(None) if keep is None else keep
        fa, fr = a64.floors(np.asarray(y32)[k], np.asarray(y64)[k])
        pa, pr = out.get(key, (0.0, 0.0))
        out[key] = (max(pa, fa), max(pr, fr))

    for N in (p64.SIZES if sizes is None else sizes):
        if N >= p64.SWITCH_N:          # the sizes either side of the kernel switch: integrate_pos' `mixed` case only
            x, t, base = p64.switch_inputs(f, N)
            y, y32 = _pair(p64.integrate64, f, x, t, base, device=device)
            e = y["edge"] | y32["edge"]
            assert e.sum() <= int(0.005 * N), (kind, "mixed", N, int(e.sum()))
            put(("integrate", kind, "mixed"), y32["xk"], y["xk"], ~e)
            continue
        if kind != "D":
            xt = p64.case_points(f, N, "vel")
            y, y32 = _pair(p64.vel64, f, xt, False, device=device)
            put(("vel", kind, "all"), y32["u"], y["u"])
            yc = p64.vel64(f, xt, False, dtype=torch.float32, device=device, chain=True)["u"]        # the other plain fp32 order (point64.FLOOR)
            put(("vel", kind, "all"), yc, y["u"])
            y, y32 = _pair(p64.vel64, f, xt, True, device=device)
            put(("vel_gated", kind, "all"), y32["u"], y["u"])
            put(("vel_gated", kind, "all"), np.where(y["inside"][:, None], yc[:, :3], 0.0), y["u"])
            assert np.array_equal(y["u"] == 0, y32["u"] == 0)
            e = y["edge"].copy()
            if N >= 31:
                assert e[:p64.N_FACE].all(), "the nine placed points sit on the gate box"
                assert y["inside"][[0, 1, 2, 3, 4, 8]].all(), "a point ON the gate box, its other coordinates inside, is inside the gate"
                e[:p64.N_FACE] = False
                assert (~y["inside"]).any()
            assert e.sum() <= int(0.005 * N), (kind, "vel", N, int(e.sum()))
            x = p64.case_points(f, N, "pos")
            for label in p64.TIME_CASES:
                if N not in p64.case_sizes(label):
                    continue
                t, base = p64.time_cases(f, N, label)
                y, y32 = _pair(p64.integrate64, f, x, t, base, device=device)
                e = y["edge"] | y32["edge"]
                assert e.sum() <= int(0.005 * N), (kind, label, N, int(e.sum()))
                assert np.array_equal(y["steps"], y32["steps"])
                put(("integrate", kind, label), y32["xk"], y["xk"], ~e)
                if label != "none":        # the other plain fp32 order (point64.FLOOR), at the sizes both integrators run
                    yc = p64.integrate64(f, x, t, base, dtype=torch.float32, device=device, chain=True)
                    ec = e | yc["edge"]
                    assert ec.sum() <= int(0.005 * N) and np.array_equal(yc["steps"], y["steps"]), (kind, label, N, int(ec.sum()))
                    put(("integrate", kind, label), yc["xk"], y["xk"], ~ec)
                st = y["steps"]
                if label == "none":
                    assert st.max() == 0 and np.array_equal(y["xk"].astype(np.float32), x)
                elif label == "one_live":
                    live = p64.one_live_points(N)
                    assert st.sum() == p64.ONE_LIVE_STEPS * len(live) and (st[live] == p64.ONE_LIVE_STEPS).all()
                elif label == "tiny":
                    assert (st == 1).all()
                elif label == "forward":
                    assert st.min() >= (4 if kind == "A" else 20)
                elif label == "mixed" and N >= 257:
                    sg = np.sign(t - base)
                    assert (sg > 0).any() and (sg < 0).any() and st.max() >= (2 if kind == "A" else 8)
                    assert (y["n_rejected"] > 0) == (kind == "B"), (kind, N, y["n_rejected"])
            q = p64.case_points(f, N, "density")
            y, y32 = _pair(p64.density64, f, q, device=device)
            put(("feat", kind, "all"), y32["feat"], y["feat"])
            put(("sigma", kind, "all"), y32["sigma"], y["sigma"])
            nf = min(p64.N_FAR, max(0, N - len(p64.SPECIAL_T)))
            if nf:
                assert (y["feat"][N - nf:] == 0).all() and (y32["feat"][N - nf:] == 0).all(), "a far point reads padding only"
                assert np.allclose(y["sigma"][N - nf:], np.log1p(np.exp(f.shift)), rtol=1e-12)
        q, view, feat = p64.case_points(f, N, "app")
        y, y32 = _pair(p64.app64, f, q, view, device=device)
        put(("app", kind, "all"), y32["rgb"], y["rgb"])
        y, y32 = _pair(p64.mlp64, f, q[:, :3], view, feat, device=device)
        put(("mlp", kind, "all"), y32, y)
        if kind == "D":
            y, y32 = _pair(p64.sh64, view, feat, device=device)
            put(("sh", kind, "all"), y32, y)
    return out


@pytest.mark.parametrize("kind", p64.KINDS)
def test_gpu_case_floors_and_edge_points(pfields, kind):
    got = gpu_case_floors(pfields, kind, sizes=p64.SIZES + ((p64.SWITCH_N + 1,) if kind != "D" else ()))     # (its first SWITCH_N points are the other call)
    bad = []
    for key, (fa, fr) in sorted(got.items()):
        rtol, atol = p64.POINT_RTOL[key], p64.POINT_ATOL[key]
        print(f"[point64] {key}: float32 floor abs {fa:.2e} rel {fr:.2e} (recorded {p64.FLOOR[key][0]:.1e} / {p64.FLOOR[key][1]:.1e}); bound atol {atol:g} rtol {rtol:g}")
        if 3 * fa > atol or 3 * fr > rtol:
            bad.append((key, fa, fr))
    assert not bad, bad
    assert {k for k in p64.FLOOR if k[1] == kind} == set(got), "a recorded floor without a case"
