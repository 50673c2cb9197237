"""tests/advect_pt64.py (the float64 yardstick of differentiable advection with per-point times, nvfi_advect_grad_pt) against
tests/golden/advect_pt.npz + advect_pt_net_*.npz - the REFERENCE's own integrate_pos under autograd on (N,1) time tensors
(tests/golden/make_golden_advect_pt.py), fields A and B - and against its defining form, advect64.advect64 per distinct time pair.  CPU only.

Cases: mixed (N = 257, the five time pairs of the scalar goldens assigned by i % 5: 0 / 1 / 3 / 2 / 8 steps on A, 0 / 1 / 3 / 8 / 9 on B, where the
surround box rejects 21 steps of inside points) and distinct (N = 97, 97 distinct pairs, 1 .. 5 steps).

Tolerance against the reference, by the rule of tests/test_advect_golden.py: the golden tensors are fp32, one plain-fp32 evaluation away from the
float64 yardstick.  That distance is measured here as advect_pt64(float32) against advect_pt64(float64) relative to the max of each tensor
(advect_pt64.GOLDEN_FLOOR: xk, gx, the worst of the 12 net tensors; asserted below to still hold), and the golden may differ from the yardstick by
at most 3 x it, not below one fp32 ulp of the tensor's scale.  Measured floors (xk / gx / worst net tensor):
  A: mixed 9.4e-8 / 1.4e-7 / 5.2e-7   distinct 6.2e-8 / 1.4e-7 / 9.7e-7      B: mixed 1.3e-7 / 2.0e-7 / 4.4e-7   distinct 1.1e-7 / 1.1e-7 / 8.9e-7
Against the grouped form the two float64 runs differ only in the order the groups' contributions are summed: 1e-12 of each tensor's max."""
import os

import numpy as np
import pytest
import torch

import advect64 as a64
import advect_pt64 as p64
import flow64 as f64
import render64 as r64
from conftest import GOLD
from helpers import load_meta

CASES = sorted(p64.GOLDEN_FLOOR)
MIXED_STEPS = {"A": [0, 1, 3, 2, 8], "B": [0, 1, 3, 8, 9]}
REJECTED = {"B:mixed": 21}


@pytest.fixture(scope="module")
def pt_gold():
    return np.load(os.path.join(GOLD, "advect_pt.npz"))


@pytest.fixture(scope="module")
def r64_fields():
    out = {}
    for kind in "AB":
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        out[kind] = r64.Field(sd, meta)
    return out


_runs = {}


def _run(fields, z, case):
    """the float64 and float32 yardstick of a golden case, computed once"""
    if case not in _runs:
        x, g, t, t1 = z[case + ":x"], z[case + ":g"], z[case + ":t"], z[case + ":t_target"]
        field = fields[case[0]]
        _runs[case] = (p64.advect_pt64(field, x, t, t1, g), p64.advect_pt64(field, x, t, t1, g, dtype=torch.float32))
    return _runs[case]


@pytest.mark.parametrize("case", CASES)
def test_yardstick_matches_reference(pt_gold, r64_fields, case):
    z, field = pt_gold, r64_fields[case[0]]
    kind, name = case.split(":")
    xc, gc, tc, t1c = p64.case_of(kind, name, field.tmax, field.tmax / (field.K - 1))
    assert all(np.array_equal(z[case + ":" + k], v) for k, v in (("x", xc), ("g", gc), ("t", tc), ("t_target", t1c))), "the fixture holds the stated inputs"
    y64, y32 = _run(r64_fields, z, case)
    assert not y64["edge"].any() and not y32["edge"].any(), np.nonzero(y64["edge"] | y32["edge"])[0]
    assert np.array_equal(y64["steps"], z[case + ":steps"]) and np.array_equal(y32["steps"], y64["steps"])
    if name == "mixed":
        assert y64["groups"] == 5 and list(y64["steps"][:5]) == MIXED_STEPS[kind]
    else:
        assert y64["groups"] == 97 and y64["steps"].min() >= 1 and y64["steps"].max() <= 5
    assert y64["n_rejected"] == y32["n_rejected"] == int(z[case + ":n_rejected"]) == REJECTED.get(case, 0)
    assert y64["n_outside"] == int(z[case + ":n_outside"])
    own = a64.floors(y32, y64)
    net = p64.golden_net(GOLD, case)
    ref = dict(xk=z[case + ":xk"], gx=z[case + ":gx"], **net)
    table = p64.GOLDEN_FLOOR[case]
    for i, what in enumerate(("xk", "gx", "worst net tensor")):
        print(f"[advect_pt golden] {case}: {what}: fp32 yardstick {own[i]:.2e} (table {table[i]:.1e}, fixture {float(z[case + ':floor'][i]):.2e})")
        assert own[i] <= table[i] * 1.02, (case, what, own[i], table[i])          # the table still states what is measured here (2 %: its rounding)
    for k in a64.KEYS:
        floor = table[0] if k == "xk" else table[1] if k == "gx" else table[2]
        err = f64.rel_err(ref[k], y64[k])
        bound = max(3 * floor, a64.ULP32)
        print(f"[advect_pt golden] {case}: {k}: max |.| {np.abs(y64[k]).max():.4g}, reference against float64 {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (case, k, err, bound)


@pytest.mark.parametrize("case", CASES)
def test_yardstick_is_the_grouped_form(pt_gold, r64_fields, case):
    """the defining property: advect64 per distinct (t, t_target) group, the net gradients summed over the groups - 1e-12 of each tensor's max - and
    the same reports"""
    z = pt_gold
    y64, _ = _run(r64_fields, z, case)
    grp = p64.grouped64(r64_fields[case[0]], z[case + ":x"], z[case + ":t"], z[case + ":t_target"], z[case + ":g"])
    for k in a64.KEYS:
        err = f64.rel_err(y64[k], grp[k])
        print(f"[advect_pt golden] {case}: {k}: against the grouped form {err:.1e}")
        assert err <= 1e-12, (case, k, err)
    assert np.array_equal(y64["edge"], grp["edge"]) and np.array_equal(y64["gated_all"], grp["gated_all"])
    assert y64["n_rejected"] == grp["n_rejected"] and y64["n_outside"] == grp["n_outside"]


def test_zero_step_points_pass_their_gradient_through(pt_gold, r64_fields):
    """the zero-step points of the mixed case (i % 5 == 0) never move and their gradient is the upstream one, in the yardstick and in the reference;
    with a scalar pair the yardstick IS advect64"""
    for case in ("A:mixed", "B:mixed"):
        z = pt_gold
        y64, _ = _run(r64_fields, z, case)
        zero = y64["steps"] == 0
        assert zero.sum() == 52 and np.array_equal(np.nonzero(zero)[0] % 5, np.zeros(52, int)) and y64["gated_all"][zero].all()
        x, g = z[case + ":x"], z[case + ":g"]
        assert np.array_equal(y64["gx"][zero], g[zero].astype(np.float64)) and np.array_equal(y64["xk"][zero], x[zero].astype(np.float64))
        assert np.array_equal(z[case + ":gx"][zero], g[zero]) and np.array_equal(z[case + ":xk"][zero], x[zero])
    field = r64_fields["A"]
    x, g = a64.case_inputs(33)
    t, t1 = p64.T_NONKEY, p64.T_NONKEY - 1.3 * field.tmax / (field.K - 1)
    a, b = p64.advect_pt64(field, x, t, t1, g), a64.advect64(field, x, t, t1, g)
    assert all(np.array_equal(a[k], b[k]) for k in a64.KEYS) and a["groups"] == 1 and (a["steps"] == 3).all()
