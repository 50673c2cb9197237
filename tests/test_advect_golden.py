"""tests/advect64.py (the float64 yardstick of differentiable advection, nvfi_advect_grad) against tests/golden/advect.npz + advect_net_*.npz: the
REFERENCE's own integrate_pos under autograd (tests/golden/make_golden_advect.py), fields A and B, N = 257.  CPU only.

Cases (T = 19/60, ts = tmax / (K - 1)): c0 t == t_target | c1 T -> T + ts/4 (1 step) | c2 T -> T - 1.3 ts (3 steps) | c3 45/60 -> +0.2 (2 steps on
A, 8 on B) | c4 0 -> 1.0 on A (8 steps), 0 -> 4.5 ts on B (9 steps).  44 of the 257 points start outside the gate of A, 98 outside the surround box
of B; the box rejects 8 / 37 / 49 steps of inside points in B's c2 / c3 / c4, the same count in float32 and float64.

Tolerance: the golden tensors are fp32, one plain-fp32 evaluation away from the float64 yardstick.  That distance is measured here, on the CPU, as
advect64(float32) against advect64(float64) relative to the max of each tensor (advect64.GOLDEN_FLOOR: xk, gx, the worst of the 12 net tensors;
asserted below to still hold), and the golden may differ from the yardstick by at most 3 x it, not below one fp32 ulp of the tensor's scale.
Measured floors (xk / gx / worst net tensor):
  A: c1 3.2e-8 / 5.4e-8 / 1.4e-6   c2 7.0e-8 / 1.1e-7 / 1.1e-6   c3 5.9e-8 / 8.9e-8 / 9.6e-7   c4 1.2e-7 / 1.2e-7 / 4.7e-7
  B: c1 2.9e-8 / 4.9e-8 / 9.0e-7   c2 7.1e-8 / 1.1e-7 / 6.0e-7   c3 1.6e-7 / 2.0e-7 / 4.3e-7   c4 1.6e-7 / 1.9e-7 / 3.3e-7;  c0: exact.
No case has a point within 4 fp32 ulp of a gate or box face at any evaluation (asserted: the yardstick's edge report is empty in both precisions)."""
import os

import numpy as np
import pytest
import torch

import advect64 as a64
import flow64 as f64
import render64 as r64
from conftest import GOLD
from helpers import load_meta

CASES = sorted(a64.GOLDEN_FLOOR)
REJECTED = {"B:c2": 8, "B:c3": 37, "B:c4": 49}
STEPS = {"A:c0": 0, "A:c1": 1, "A:c2": 3, "A:c3": 2, "A:c4": 8, "B:c0": 0, "B:c1": 1, "B:c2": 3, "B:c3": 8, "B:c4": 9}


@pytest.fixture(scope="module")
def adv_gold():
    return np.load(os.path.join(GOLD, "advect.npz"))


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


@pytest.mark.parametrize("case", CASES)
def test_yardstick_matches_reference(adv_gold, r64_fields, case):
    z, field = adv_gold, r64_fields[case[0]]
    x, g, t, t1 = z[case + ":x"], z[case + ":g"], float(z[case + ":t"]), float(z[case + ":t_target"])
    xc, gc = a64.case_inputs(257)
    assert np.array_equal(x, xc) and np.array_equal(g, gc)
    y64 = a64.advect64(field, x, t, t1, g)
    y32 = a64.advect64(field, x, t, t1, g, dtype=torch.float32)
    assert not y64["edge"].any() and not y32["edge"].any(), np.nonzero(y64["edge"])[0]
    assert len(y64["steps"]) == int(z[case + ":steps"]) == STEPS[case]
    assert y64["n_rejected"] == y32["n_rejected"] == int(z[case + ":n_rejected"]) == REJECTED.get(case, 0)
    assert y64["n_outside"] == int(z[case + ":n_outside"]) == (44 if case[0] == "A" else 98)
    own = a64.floors(y32, y64)
    net = a64.golden_net(GOLD, case)
    ref = dict(xk=z[case + ":xk"], gx=z[case + ":gx"])
    for k in a64.NET_NAMES:
        ref[k] = np.zeros_like(y64[k], dtype=np.float32) if net is None else net[k]
    table = a64.GOLDEN_FLOOR[case]
    for i, what in enumerate(("xk", "gx", "worst net tensor")):
        print(f"[advect golden] {case}: {what}: fp32 yardstick {own[i]:.2e} (table {table[i]:.1e}, fixture {float(z[case + ':floor'][i]):.2e})")
        assert own[i] <= table[i] * 1.02, (case, what, own[i], table[i])          # the table still states what is measured here (2 %: its rounding)
    for k in a64.KEYS:
        floor = table[0] if k == "xk" else table[1] if k == "gx" else table[2]
        err = f64.rel_err(ref[k], y64[k])
        bound = max(3 * floor, a64.ULP32) if floor > 0 else 0.0
        print(f"[advect golden] {case}: {k}: max |.| {np.abs(y64[k]).max():.4g}, reference against float64 {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (case, k, err, bound)
    if case.endswith("c0"):
        assert np.array_equal(y64["xk"], x.astype(np.float64)) and np.array_equal(y64["gx"], g.astype(np.float64))


def test_schedule_is_flow64s(r64_fields):
    """advect64.schedule is flow64.schedule's loop with the target given: the same steps wherever fp32(t) + fp32(dt) lands on fp32(t_target), and
    the limit of 64 steps is the same refusal"""
    for kind, field in r64_fields.items():
        ts = field.tmax / (field.K - 1)
        n = 0
        for t, dt in ((19.0 / 60.0, ts / 4), (19.0 / 60.0, -1.3 * ts), (0.75, 0.2), (0.0, 1.0), (0.0, 4.5 * ts), (0.25, 0.0)):
            if np.float32(np.float32(t) + np.float32(dt)) == np.float32(t + dt):
                assert a64.schedule(field, t, t + dt) == f64.schedule(field, t, dt), (kind, t, dt)
                n += 1
        assert n >= 3
        assert len(a64.schedule(field, 0.0, 31.75 * ts)) == 64          # 63 full steps and a remainder (32 ts leaves one more, of rounding)
        with pytest.raises(ValueError):
            a64.schedule(field, 0.0, 32.25 * ts)


def test_gated_points_pass_their_gradient_through(adv_gold, r64_fields):
    """a point outside the gate at every evaluation never moves, and its gradient is the upstream one, in the yardstick and in the reference"""
    for case in ("A:c2", "B:c2"):
        z = adv_gold
        y = a64.advect64(r64_fields[case[0]], z[case + ":x"], float(z[case + ":t"]), float(z[case + ":t_target"]), z[case + ":g"])
        ga = y["gated_all"]
        assert ga.sum() == (44 if case[0] == "A" else 98)
        assert np.array_equal(y["gx"][ga], z[case + ":g"][ga].astype(np.float64)) and np.array_equal(y["xk"][ga], z[case + ":x"][ga].astype(np.float64))
        assert np.array_equal(z[case + ":gx"][ga], z[case + ":g"][ga]) and np.array_equal(z[case + ":xk"][ga], z[case + ":x"][ga])
