"""tests/flow64.py (the float64 yardstick of the flow branch, nvfi_render_flow) against tests/golden/flow.npz: maps composited from the
REFERENCE's own field.vel and field.integrate_pos at the appearance-masked samples of its own test-mode renders
(tests/golden/make_golden_flow.py), on fields A and B, camera of the render_eval goldens.  CPU only.

Cases: c1 non-key t, dt = +ts/4 | c2 dt = -1.3 ts (three steps) | c3 key t, dt = +ts/2 | c4 t = 45/60, dt = +0.2 (leaves tmax; 2 steps on A,
8 on B) | c5 the weights of a transfer_vel render | c6 dt = 0 | c7 (B) dt = +1.5 ts: 29 steps of points inside the surround box rejected
(c2: 191, c4: 399, c1: 2, c3: 3, c5: 8 - every non-zero case of field B has some).

Tolerance: the golden maps are fp32, so they sit one plain-fp32 evaluation away from the float64 yardstick.  That distance is measured here,
on the CPU, as flow64(float32) against flow64(float64) relative to max |map|, per case and map (flow64.GOLDEN_FLOOR, asserted below to still
hold), and the golden may differ from the yardstick by at most 4 x it.  Measured floors (vel_map / flow_map / flow2d):
  A: c1 2.8e-7 / 2.5e-7 / 2.7e-6   c2 2.8e-7 / 1.8e-7 / 5.2e-7   c3 2.4e-7 / 2.8e-7 / 1.1e-6   c4 2.5e-7 / 2.5e-7 / 6.9e-7   c5 2.1e-7 / 3.0e-7 / 2.5e-6
  B: c1 3.2e-7 / 7.4e-7 / 9.6e-6   c2 3.2e-7 / 4.1e-7 / 1.6e-6   c3 2.7e-7 / 4.5e-7 / 3.6e-6   c4 3.9e-7 / 2.5e-7 / 6.1e-7   c5 3.3e-7 / 5.7e-7 / 6.9e-6
     c7 3.2e-7 / 4.4e-7 / 1.1e-6;  c6 (dt = 0): vel_map as c1, the other two exactly zero.
flow2d's floor is the largest where dt is smallest: pi(P') - pi(P) is a difference of two pixel positions.  max |map| per case is recorded in
the fixture (vel_map 1.4 - 2.2 world units per unit time, flow_map 0.03 - 0.46, flow2d 8 - 134 pixels): the signal is not tiny.
No case has a sample within 4 fp32 ulp of a gate or box face (asserted: the yardstick's edge report is empty in float64 and float32)."""
import os

import numpy as np
import pytest
import torch

import flow64 as f64
import render64 as r64
from conftest import GOLD
from helpers import load_meta

CASES = sorted(f64.GOLDEN_FLOOR)


@pytest.fixture(scope="module")
def flow_gold():
    return np.load(os.path.join(GOLD, "flow.npz"))


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


_cache = {}


def _yard(gold, flow_gold, fields, case, dtype):
    """computed once per (case, dtype) and shared"""
    if (case, dtype) not in _cache:
        kind = case[0]
        cam = (flow_gold[f"{kind}:pose"], int(flow_gold[f"{kind}:H"]), int(flow_gold[f"{kind}:W"]), float(flow_gold[f"{kind}:focal"]))
        w = flow_gold[str(flow_gold[case + ":wkey"])]
        _cache[(case, dtype)] = f64.flow64(fields[kind], gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"], float(flow_gold[case + ":t"]),
                                           float(flow_gold[case + ":dt"]), w, cam, dtype=dtype)
    return _cache[(case, dtype)]


@pytest.mark.parametrize("case", CASES)
def test_yardstick_matches_reference(gold, flow_gold, r64_fields, case):
    y64 = _yard(gold, flow_gold, r64_fields, case, torch.float64)
    y32 = _yard(gold, flow_gold, r64_fields, case, torch.float32)
    assert len(y64["edge_samples"]) == 0 and len(y32["edge_samples"]) == 0, y64["edge_samples"]
    assert y64["M"] == int(flow_gold[case + ":M"]) and y64["n_rejected"] == int(flow_gold[case + ":n_rejected"])
    for k, floor in zip(f64.MAP_KEYS, f64.GOLDEN_FLOOR[case]):
        own = f64.rel_err(y32[k], y64[k])
        err = f64.rel_err(flow_gold[f"{case}:{k}"], y64[k])
        print(f"[flow golden] {case}:{k}: max |map| {np.abs(y64[k]).max():.4g}, fp32 yardstick {own:.2e} (table {floor:.1e}), reference {err:.2e}")
        assert own <= floor * 1.02, (case, k, own, floor)            # the table still states what is measured here (2 %: its rounding)
        assert err <= 4 * floor, (case, k, err, floor)
    if float(flow_gold[case + ":dt"]) == 0.0:
        assert not y64["flow_map"].any() and not y64["flow2d"].any()
        assert not flow_gold[case + ":flow_map"].any() and not flow_gold[case + ":flow2d"].any()
    else:
        assert np.abs(y64["flow_map"]).max() > 1e-3 * abs(float(flow_gold[case + ":dt"])) and np.abs(y64["flow2d"]).max() > 1e-3


def test_rejected_step_case(flow_gold):
    assert int(flow_gold["B:c7:n_rejected"]) >= 1


@pytest.mark.parametrize("kind", "AB")
def test_flow_over_dt_tends_to_velocity(gold, flow_gold, r64_fields, kind):
    """flow_map / dt -> vel_map as dt -> 0: the distance shrinks with dt (by more than 0.6 per step of the list) and at dt = 1e-4 it is
    below 1e-3 of the map (the field's velocities change over times of order 0.1)"""
    case = f"{kind}:c1"
    w = flow_gold[str(flow_gold[case + ":wkey"])]
    o, d, t = gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"], float(flow_gold[case + ":t"])
    prev = None
    for dt in (4e-3, 1e-3, 1e-4):
        y = f64.flow64(r64_fields[kind], o, d, t, dt, w, None, want=("vel", "flow"))
        dt32 = -y["steps"][0][1]          # the fp32 step the integrator took
        e = f64.rel_err(y["flow_map"] / dt32, y["vel_map"])
        assert prev is None or e < 0.6 * prev, (dt, e, prev)
        prev = e
    assert prev < 1e-3, prev


def test_flow_to_rgb():
    """shape, range and the four axis colours of the HSV wheel (u right, v down): red, yellow-green, cyan, blue-violet; no motion is white"""
    from nvfi_amd.utils.flow_vis import flow_to_rgb
    f = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]], [[0.0, -1.0], [0.0, 0.0], [0.3, 0.0]]])
    rgb = flow_to_rgb(f)
    assert rgb.shape == (2, 3, 3) and float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
    want = torch.tensor([[[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.0, 1.0, 1.0]], [[0.5, 0.0, 1.0], [1.0, 1.0, 1.0], [1.0, 0.7, 0.7]]])
    assert torch.allclose(rgb, want, atol=1e-6), rgb
    assert torch.allclose(flow_to_rgb(f, max_mag=2.0)[0, 0], torch.tensor([1.0, 0.5, 0.5]), atol=1e-6)
    assert torch.equal(flow_to_rgb(torch.zeros(4, 5, 2)), torch.ones(4, 5, 3))


def test_abi_refusals_need_no_device():
    """the refusals nvfi_render_flow decides on the host, before anything is launched: R <= 0 returns 0; a call without NVFI_WANT_FLOW, a
    train-mode call and a field without a velocity net return error 2"""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    assert _lib.NVFI_WANT_FLOW == 32 and L.nvfi_abi_version() == 5

    def call(desc, R, flags):
        return L.nvfi_render_flow(C.byref(desc), C.c_int64(R), None, None, C.c_float(0.3), C.c_float(0.1), C.c_int(flags), None, None, C.c_int(0),
                                  C.c_int(0), C.c_float(1.0), None, None, None, None, C.c_int64(0), C.c_void_p(0))
    d = _lib.FieldDesc()
    d.use_vel = 1
    assert call(d, 0, _lib.NVFI_WANT_FLOW) == 0 and call(d, -3, 0) == 0
    assert call(d, 4, 0) == 2 and b"NVFI_WANT_FLOW" in L.nvfi_last_error()
    assert call(d, 4, _lib.NVFI_WANT_FLOW | _lib.NVFI_TRAIN) == 2 and b"NVFI_TRAIN" in L.nvfi_last_error()
    d.use_vel = 0
    assert call(d, 4, _lib.NVFI_WANT_FLOW) == 2 and b"use_vel" in L.nvfi_last_error()
