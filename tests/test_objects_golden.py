"""The float64 yardstick of the object branches (tests/objects64.py) against the fixture captured from the reference (tests/golden/objects.npz,
written by tests/golden/make_golden_objects.py), on the CPU, and the ABI surface of the two calls.

Layer maps: the yardstick (float64, on the fixture's weight map) against the maps composited from the reference's own weights, colours and masks,
relative to max |map|, within 4 x the case's plain-fp32 floor objects64.GOLDEN_FLOOR (the reference IS a plain fp32 evaluation); the floor is
measured again here and must not exceed its entry.  Selected renders: rgb, depth, acc, weight by the rule of tests/test_gpu_render64.py
(objects64.MAP_RTOL x |ref| + helpers.FP32_FLOOR element-wise); rays with a sample in the near-threshold report may be set aside, at most 2 %."""
import os
import re

import numpy as np
import pytest
import torch

import objects64 as o64
import render64 as r64
from conftest import GOLD, ROOT
from helpers import FP32_FLOOR, load_meta

CASES = sorted(o64.GOLDEN_FLOOR)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "objects.npz"))


def mask_state(fx, kind):
    """the fixture's MaskField state_dict of a field: field B stores its own head and shares field A's trunk"""
    sd = {k[len("A:mask:"):]: fx[k] for k in fx.files if k.startswith("A:mask:")}
    sd.update({k[len(kind) + 6:]: fx[k] for k in fx.files if k.startswith(kind + ":mask:")})
    return sd


_ctx = {}


def context(fx, gold, kind):
    if kind not in _ctx:
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        _ctx[kind] = (r64.Field(sd, meta), o64.mask_params(mask_state(fx, kind)), gold[f"{kind}:rays_o"][::2], gold[f"{kind}:rays_d"][::2],
                      bool(meta["white_background"]))
    return _ctx[kind]


_runs = {}


def run(fx, gold, case):
    if case not in _runs:
        field, mp, o, d, white = context(fx, gold, case[0])
        t, sel, w = float(fx[case + ":t"]), fx[case + ":select"], fx[case + ":weight"]
        _runs[case] = (o64.objects64(field, mp, o, d, t, white, select=sel, weights=w),
                       o64.objects64(field, mp, o, d, t, white, select=sel, weights=w, dtype=torch.float32))
    return _runs[case]


@pytest.mark.parametrize("case", CASES)
def test_yardstick_reproduces_fixture(fx, gold, case):
    y64, y32 = run(fx, gold, case)
    R = y64["acc"].shape[0]
    measured = o64.layer_floor(y32, y64)
    for i, k in enumerate(o64.LAYER_KEYS):
        floor = o64.GOLDEN_FLOOR[case][i]
        err = o64.rel_err(fx[f"{case}:{k}"], y64[k])
        print(f"[objects] {case}:{k}: reference {err:.2e}, fp32 yardstick {measured[i]:.2e}, floor {floor:.2e}, bound {4 * floor:.2e}")
        assert measured[i] <= floor, (case, k, measured[i], floor)
        assert err <= 4 * floor, (case, k, err, 4 * floor)
    assert o64.rel_err(fx[case + ":mask_map"], y64["obj_acc"]) <= 4 * o64.GOLDEN_FLOOR[case][1]
    near = np.union1d(y64["near_rays"], y32["near_rays"])
    for name, got in (("reference", {k: fx[f"{case}:{k}"] for k in o64.MAP_KEYS}), ("fp32 yardstick", y32)):
        bad = o64.map_failures(got, y64, FP32_FLOOR)
        aside = np.unique(np.concatenate(list(bad.values()))) if bad else np.zeros(0, np.int64)
        print(f"[objects] {case}: {name}: rays set aside {len(aside)}/{R} (near-threshold rays {len(near)})")
        assert np.isin(aside, near).all(), (case, name, bad)
        assert len(aside) <= o64.MAX_ASIDE * R, (case, name, len(aside))


@pytest.mark.parametrize("case", ["A:nr", "B:nf"])
def test_layer_identity_float64(fx, gold, case):
    """sum_k obj_rgb = the colour before background and clamp; sum_k obj_acc = sum of the masked weights; in float64 to its rounding"""
    y64, _ = run(fx, gold, case)
    w = np.where(y64["mask"], fx[case + ":weight"].astype(np.float64), 0.0)
    assert np.abs(y64["obj_rgb"].sum(1) - y64["pre_rgb"]).max() <= 1e-13
    assert np.abs(y64["obj_acc"].sum(1) - w.sum(1)).max() <= 1e-13
    assert not y64["obj_rgb"][~y64["mask"].any(1)].any()


@pytest.mark.parametrize("kind", "AB")
def test_select_ones_is_the_plain_render(fx, gold, kind):
    field, mp, o, d, white = context(fx, gold, kind)
    t = float(fx[f"{kind}:no:t"])
    y = o64.objects64(field, mp, o, d, t, white, select=np.ones(len(mp[9]), np.float32))
    assert np.abs(y["s"] - 1.0).max() <= 1e-14
    ref = r64.render64(field, o, d, t, None, white, grads=False)
    for k in o64.MAP_KEYS:
        assert np.abs(y[k] - ref[k]).max() <= 1e-12, k
    plain = o64.objects64(field, mp, o, d, t, white, select=None)
    for k in o64.MAP_KEYS:
        assert np.array_equal(plain[k], ref[k]) or np.abs(plain[k] - ref[k]).max() <= 1e-15, k


def test_exports_and_header():
    """both new symbols are exported by the built library and declared in the header"""
    from nvfi_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    for name in ("nvfi_render_objects", "nvfi_render_fwd_select"):
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+NVFI_WANT_SELECT\s+64\b", hdr) and _lib.NVFI_WANT_SELECT == 64
