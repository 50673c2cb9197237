"""Differentiable field lookups, CPU side: the float64 yardstick (tests/lookup64.py) against goldens made from the reference's
compute_densityfeature / compute_appfeature under autograd (tests/golden/make_golden_lookup.py), and the presence of the feature at every layer
(header, library, binding, field methods).

Bound of every comparison, per tensor (value, g_xyzt, each plane gradient, basis_mat's): |got - ref64| <= max(3 x floor, 1e-5 x max |ref64|) with
floor = max |yardstick(float32) - yardstick(float64)| on the same case - lookup64.bound, the rule of tests/test_gpu_lookup.py.  Measured here
(reference - yardstick / float32 floor / bound, worst tensor relative to its bound): density value 1.8e-6 / 1.3e-6 / 8.8e-5, density g_xyzt
2.4e-5 / 2.3e-5 / 1.2e-4 (field B; the worst, 0.21 of its bound), plane gradients 2e-7 .. 8e-7 / the same / 2e-6 .. 8e-6, appearance value
4.8e-9 / 4.8e-9 / 4.5e-8, basis_mat 3.5e-8 / 3.1e-8 / 5.2e-7.  The wrong variants leave the bound by factors of 1e3 and more."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import lookup64 as l64
import render64 as r64
from conftest import GOLD, ROOT
from helpers import load_meta

SYMBOLS = ("nvfi_density_grad", "nvfi_appfeat_at", "nvfi_appfeat_grad")
_cache = {}


@pytest.fixture(scope="module")
def lg():
    return np.load(os.path.join(GOLD, "lookup.npz"))


def golden_field(kind):
    if kind not in _cache:
        meta, sd = load_meta(kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        _cache[kind] = (r64.Field(sd, meta), [int(g) for g in meta["gridSize"]])
    return _cache[kind]


def yardsticks(lg, kind, family):
    """(float64, float32, wrong float64) results of a golden case, computed once"""
    key = (kind, family)
    if key not in _cache:
        field, _ = golden_field(kind)
        fn = l64.density_lookup64 if family == "density" else l64.app_lookup64
        q, g = lg[f"{kind}:xyzt"], lg[f"{kind}:{family}:g"]
        _cache[key] = (fn(field, q, g), fn(field, q, g, dtype=torch.float32), fn(field, q, g, wrong=True))
    return _cache[key]


def golden_tensors(lg, kind, family):
    names = l64.D_NAMES if family == "density" else l64.A_NAMES
    out = {"value": lg[f"{kind}:{family}:value"], "g_xyzt": lg[f"{kind}:{family}:g_xyzt"]}
    out.update({"grad:" + n: lg[f"{kind}:{family}:grad:{n}"] for n in names})
    return out


@pytest.mark.parametrize("family", ["density", "app"])
@pytest.mark.parametrize("kind", ["A", "B"])
def test_yardstick_reproduces_reference_goldens(lg, kind, family):
    y64, y32, _ = yardsticks(lg, kind, family)
    t64, t32, ref = l64.tensors(y64), l64.tensors(y32), golden_tensors(lg, kind, family)
    assert set(t64) == set(ref)
    for label in t64:
        e, b = l64.max_err(ref[label], t64[label]), l64.bound(t64[label], t32[label])
        print(f"{kind}:{family}:{label}: reference - yardstick {e:.2e}, float32 floor {l64.max_err(t32[label], t64[label]):.2e}, bound {b:.2e}")
        assert np.abs(t64[label]).max() > 0, (kind, family, label, "nothing to compare")
        assert e <= b, (kind, family, label, e, b)


@pytest.mark.parametrize("kind", ["A", "B"])
def test_wrong_variants_are_outside_the_bound(lg, kind):
    """density: the t' gradient scaled by K / 2 - only column 3 of g_xyzt moves; appearance: a space plane's share without the time plane of its
    index - its gradient and the spatial coordinate gradients move, the values and the time planes' gradients do not"""
    y64, y32, bad = yardsticks(lg, kind, "density")
    ref = golden_tensors(lg, kind, "density")
    b = l64.bound(y64["g_xyzt"], y32["g_xyzt"])
    assert l64.max_err(ref["g_xyzt"][:, 3], bad["g_xyzt"][:, 3]) > 3 * b
    assert np.array_equal(bad["g_xyzt"][:, :3], y64["g_xyzt"][:, :3]) and np.array_equal(bad["value"], y64["value"])
    y64, y32, bad = yardsticks(lg, kind, "app")
    ref = golden_tensors(lg, kind, "app")
    t64, t32, tb = l64.tensors(y64), l64.tensors(y32), l64.tensors(bad)
    for label in ["g_xyzt"] + [f"grad:app_plane_space.{i}" for i in range(3)]:
        assert l64.max_err(ref[label], tb[label]) > 3 * l64.bound(t64[label], t32[label]), (kind, label)
    for label in ["value", "grad:basis_mat.weight"] + [f"grad:app_plane_time.{i}" for i in range(3)]:
        assert l64.max_err(tb[label], t64[label]) <= l64.bound(t64[label], t32[label]), (kind, label)


@pytest.mark.parametrize("kind", ["A", "B"])
def test_restated_lookup_is_render64_planes(lg, kind):
    """lookup64.planes is render64._planes (F.grid_sample) wherever no cell decision is in question: the golden points that are not texel nodes"""
    field, grid = golden_field(kind)
    q = lg[f"{kind}:xyzt"]
    keep = (l64.texel_distance(q, grid, field.K) >= 1e-4).all(1)
    assert 40 <= keep.sum() < len(q)
    x4 = torch.from_numpy(q[keep]).double()
    P = {k: v.double() for k, v in field.p32.items()}
    for which in ("density", "app"):
        with torch.no_grad():
            a, b = l64.planes(P, which, x4), r64._planes(P, which, x4)
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_golden_points_meet_their_conditions(lg):
    for kind in ("A", "B"):
        field, grid = golden_field(kind)
        q = lg[f"{kind}:xyzt"]
        assert q.shape == (96, 4) and q.dtype == np.float32
        d = l64.texel_distance(q, grid, field.K)
        node = d < 1e-4
        assert (d[node] == 0).all(), "a coordinate is either ON a texel node or 1e-4 away from every node"
        assert node[:, :3].sum() >= 6 and node[:, 3].sum() >= 4
        for c in range(3):
            assert (q[:, c] == -1).any() and (q[:, c] == 1).any() and ((q[:, c] == 0).any() or grid[c] % 2 == 0)
        assert (np.abs(q[:, :3]) > 1.05).any() and np.abs(q[:, :3]).max() <= 1.15
        assert (q[:, 3] < -1).any() and (q[:, 3] > 1).any()
        frac = d[:, 3] >= 1e-4
        assert frac.sum() >= 30 and (~frac).sum() >= 10, "integer and fractional time rows"
        for family in ("density", "app"):
            assert np.abs(lg[f"{kind}:{family}:g_xyzt"]).max(0).min() > 0, "all four columns carry a gradient"


def test_dead_lookups_are_exact_zeros():
    """far, non-finite and wholly outside points: value 0, every gradient 0 (nothing NaN reaches the graph)"""
    field, _ = golden_field("A")
    q = np.array([[1e6, 0, 0, 0], [0, -1e6, 0, 0], [np.nan, 0, 0, 0], [0, 0, np.inf, 0], [0, 0, 0, -np.inf], [0.1, 0.2, 0.3, np.nan],
                  [1.5, 1.5, 1.5, 0.0], [0.1, 0.2, 0.3, 50.0], [3e38, 3e38, -3e38, 3e38]], np.float32)
    for dtype in (torch.float64, torch.float32):
        y = l64.density_lookup64(field, q, np.ones(len(q), np.float32), dtype=dtype)
        assert not y["value"].any() and not y["g_xyzt"].any() and all(not g.any() for g in y["grads"].values())
        y = l64.app_lookup64(field, q, np.ones((len(q), 32), np.float32), dtype=dtype)
        assert not y["value"].any() and not y["g_xyzt"].any() and all(not g.any() for g in y["grads"].values())


def test_header_library_and_binding():
    from nvfi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert re.search(r"#define NVFI_ABI_VERSION 5\b", hdr)
    assert re.search(r"int\s+nvfi_density_grad\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*xyzt.*?const float\*\s*g_feat.*?float\*\s*g_xyzt"
                     r".*?const nvfi_grads\*\s*grads.*?void\*\s*stream\)\s*;", hdr, re.S)
    assert re.search(r"int\s+nvfi_appfeat_at\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*xyzt,\s*float\*\s*feat.*?void\*\s*stream\)\s*;", hdr, re.S)
    assert re.search(r"int\s+nvfi_appfeat_grad\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*xyzt,\s*const float\*\s*g_feat.*?float\*\s*g_xyzt"
                     r".*?const nvfi_grads\*\s*grads.*?void\*\s*stream\)\s*;", hdr, re.S)
    assert os.path.exists(_lib.SO), "libnvfi_hip.so has not been built"
    L = C.CDLL(_lib.SO)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.nvfi_abi_version() == 5
    from nvfi_amd.build import SOURCES
    assert "lookup.hip" in SOURCES
    from nvfi_amd.utils import field_lookup as fl
    assert all(callable(getattr(fl, n)) for n in ("density_grad_raw", "appfeat_raw", "appfeat_grad_raw"))


def test_refused_before_anything_is_launched():
    """N >= 2^31 - 256 and a descriptor check_desc rejects: error 2 with a message, before the first HIP call - this runs without a GPU, on a
    host-built descriptor and dummy pointers that nothing may dereference; an empty call is a no-op"""
    from nvfi_amd import _lib
    from test_abi_and_host import _plan_desc
    L = _lib.lib()
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)
    G = _lib.Grads()
    calls = {
        "nvfi_density_grad": lambda d, n: L.nvfi_density_grad(C.byref(d), C.c_int64(n), p, p, p, C.byref(G), None),
        "nvfi_appfeat_at": lambda d, n: L.nvfi_appfeat_at(C.byref(d), C.c_int64(n), p, p, None),
        "nvfi_appfeat_grad": lambda d, n: L.nvfi_appfeat_grad(C.byref(d), C.c_int64(n), p, p, p, C.byref(G), None),
    }

    def refused(rc, *words):
        msg = L.nvfi_last_error().decode()
        assert rc == 2 and all(w in msg for w in words), (rc, msg)

    d = _plan_desc()
    for name, call in calls.items():
        for n in ((1 << 31) - 256, 1 << 31, 1 << 40):
            refused(call(d, n), name, "N too large")
        assert call(d, 0) == 0 and call(d, -3) == 0
    d.Cd = 16
    for name, call in calls.items():
        refused(call(d, 16), "Cd=16")
        refused(call(d, 0), "Cd=16")            # the descriptor is checked before the empty call returns 0
    assert not any(dummy), "a refused call wrote through its pointers"


def test_field_methods_exist_and_refuse_the_cpu():
    from helpers import make_model
    from nvfi_amd import _lib
    from nvfi_amd.models import NVFi
    from nvfi_amd.models.tensorf_keyframe import TensorVMKeyframeTimeKplane
    for cls in (TensorVMKeyframeTimeKplane, NVFi):
        for name in ("lookup_density", "lookup_appfeature", "compute_appfeature"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    m, _ = make_model("A", device="cpu")
    q = torch.rand(8, 4) * 2 - 1
    for obj in (m.nvfi, m):
        for name in ("lookup_density", "lookup_appfeature", "compute_appfeature"):
            with pytest.raises(_lib.NvfiError):
                getattr(obj, name)(q)
            with pytest.raises(_lib.NvfiError):
                getattr(obj, name)(q.clone().requires_grad_(True))
