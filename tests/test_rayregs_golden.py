"""Distortion loss on ray weights, CPU side: the presence of the feature at every layer (ABI, header, binding, utils, drivers) and the float64
yardstick (tests/raydist64.py) against itself - its explicit-midpoint form against the index form the kernel computes, its autograd gradient
against the closed form, the stored float64 results, the stored fp32 floors - and the blind-spot checks, made on the very rows the GPU tests upload."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import raydist64 as r64
from conftest import GOLD, ROOT


@pytest.fixture(scope="module")
def gr():
    return np.load(os.path.join(GOLD, "rayregs.npz"))


def _case(case, R, S):
    seed = r64.CASES.index(case) * 100 + S
    return (r64.named_case(case, R, S, seed),) + r64.geometry(R, S, seed)


def test_exports_and_header():
    from nvfi_amd import _lib
    from nvfi_amd.build import SOURCES
    assert "raydist.hip" in SOURCES
    assert "nvfi_ray_distortion" in _lib.EXPORTS and "nvfi_ray_distortion_workspace_bytes" in _lib.EXPORTS
    assert os.path.exists(_lib.SO), "libnvfi_hip.so has not been built"
    L = _lib.lib()      # the binding's table gives both functions their argtypes: plain numbers below
    assert hasattr(L, "nvfi_ray_distortion") and hasattr(L, "nvfi_ray_distortion_workspace_bytes") and L.nvfi_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert "int nvfi_ray_distortion(" in header and "int nvfi_ray_distortion_workspace_bytes(" in header
    # the workspace query is host code: it answers without a GPU, and refuses what it cannot size
    n = ctypes.c_int64(-1)
    assert L.nvfi_ray_distortion_workspace_bytes(2048, ctypes.byref(n)) == 0 and n.value >= 2048 * 8
    assert L.nvfi_ray_distortion_workspace_bytes(-1, ctypes.byref(n)) == 2


def test_python_surface():
    from nvfi_amd import _lib, utils
    from nvfi_amd.models import NVFi
    from nvfi_amd.models.tensorf_keyframe import TensorVMKeyframeTimeKplane
    from nvfi_amd.utils import ray_regs
    from nvfi_amd.utils.evaluation_utils import render_test_evaluation
    assert utils.distortion_loss is ray_regs.distortion_loss and utils.distortion_loss_raw is ray_regs.distortion_loss_raw
    assert list(inspect.signature(ray_regs.distortion_loss).parameters) == ["weights", "delta"]
    sig = inspect.signature(ray_regs.distortion_loss_raw).parameters
    assert list(sig)[:6] == ["weights", "delta", "grad_scale", "grad_scale_dev", "out", "want_per_ray"]
    assert sig["grad_scale"].default == 1.0 and sig["grad_scale_dev"].default is None and sig["want_per_ray"].default is False
    with pytest.raises(_lib.NvfiError):
        utils.distortion_loss(torch.rand(4, 8), 0.01)
    with pytest.raises(_lib.NvfiError):
        utils.distortion_loss_raw(torch.rand(4, 8), 0.01)
    sig = inspect.signature(TensorVMKeyframeTimeKplane.render_mse_backward_).parameters
    assert sig["distortion_weight"].default == 0.0 and isinstance(sig["distortion_weight"].default, float)
    sig = inspect.signature(render_test_evaluation).parameters
    assert sig["with_distortion"].default is False
    for cls in (TensorVMKeyframeTimeKplane, NVFi):
        assert callable(getattr(cls, "distortion_delta")) and callable(getattr(cls, "distortion_loss"))


def test_distortion_delta_is_step_over_the_ray_range():
    from helpers import make_model
    model, meta = make_model("A", device="cpu")
    f = model.nvfi
    want = float(f.stepSize) / (float(meta["far"]) - float(meta["near"]))
    assert f.distortion_delta() == pytest.approx(want, rel=1e-7) and model.distortion_delta() == f.distortion_delta()
    assert 0.0 < f.distortion_delta() * f.nSamples < 4.0


@pytest.mark.parametrize("case", r64.CASES)
def test_midpoint_form_equals_index_form(case):
    """two jitters and two t_min: they cancel, the explicit intervals give delta * |i - j| to 1e-13 relative"""
    R, S = 5, 129
    w, t_min, u, step = _case(case, R, S)
    z = r64.index_form(w, r64.delta_of(step))
    for tm, uu in ((t_min, u), (t_min + 0.37, u), (t_min, np.full(R, 0.0)), (np.full(R, r64.NEAR), 1.0 - u)):
        y = r64.distortion(w, tm, step, uu)
        e = r64.errors(z["loss"], z["grad"], z["per_ray"], y)
        print(case, e)
        assert max(e) <= 1e-13, (case, e)


@pytest.mark.parametrize("case", r64.CASES)
def test_autograd_gradient_is_the_closed_form(case):
    """A_i = sum_{j<i} (i - j) w_j and B_i from the right by explicit loops: d loss / d w_i = (delta / R) [2 (A_i + B_i) + 2/3 w_i]"""
    R, S = 5, 65
    w, t_min, u, step = _case(case, R, S)
    y = r64.distortion(w, t_min, step, u)
    delta, w64 = r64.delta_of(step), w.astype(np.float64)
    g = np.empty((R, S))
    for r in range(R):
        for i in range(S):
            A = sum((i - j) * w64[r, j] for j in range(i))
            B = sum((j - i) * w64[r, j] for j in range(i + 1, S))
            g[r, i] = delta / R * (2.0 * (A + B) + 2.0 / 3.0 * w64[r, i])
    assert r64._rel(g, y["grad"]) <= 1e-13
    # and it is the derivative: central differences of the float64 loss (a quadratic form: exact up to rounding)
    h = 1e-4
    for (r, i) in ((0, 0), (2, S // 2), (4, S - 1)):
        e = np.zeros((R, S))
        e[r, i] = h
        fd = (r64.distortion(w64 + e, t_min, step, u)["loss"] - r64.distortion(w64 - e, t_min, step, u)["loss"]) / (2 * h)
        assert abs(fd - y["grad"][r, i]) <= 1e-9 * np.abs(y["grad"]).max()


def test_named_properties_of_the_cases():
    R, S = 5, 65
    w, t_min, u, step = _case("spike", R, S)
    y = r64.distortion(w, t_min, step, u)
    assert ((w != 0).sum(1) == 1).all() and w[0, -1] != 0 and w[1, 0] != 0
    want = r64.delta_of(step) * w.astype(np.float64).max(1) ** 2 / 3.0                  # D_r = delta w^2 / 3
    assert np.abs(y["per_ray"] - want).max() <= 1e-13 * want.max()      # (the width is a float64 difference of two interval ends)
    w, t_min, u, step = _case("zeros", R, S)
    y = r64.distortion(w, t_min, step, u)
    assert not w[1].any() and not w[4].any() and w[0].any()
    assert y["per_ray"][1] == 0.0 and not y["grad"][1].any()
    w = _case("opaque", R, S)[0]
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    w = _case("two_surfaces", R, 129)[0]
    assert w[0, 64] > 0.2 and w[0, 64] > 10 * w[0, 63]                                     # the sharp surface sits on the chunk boundary
    assert w[:, -1].min() > 1e-4                                                           # alpha is kept on the last sample
    w = _case("fog", R, S)[0]
    assert w.max() < 0.1 and (w > 0).all()
    # rays repeat with period PERIOD: what lets the yardstick run once per distinct ray
    w = r64.named_case("fog", 30, 7, 3)
    assert np.array_equal(w[:r64.PERIOD], w[r64.PERIOD:2 * r64.PERIOD]) and not np.array_equal(w[0], w[1])


@pytest.mark.parametrize("case", r64.CASES)
def test_yardstick_reproduces_the_stored_results(gr, case):
    for (R, S) in r64.SMALL:
        key = f"{case}:{R}x{S}"
        w, t_min, u, step = _case(case, R, S)
        assert np.array_equal(w, gr[key + ":w"]) and np.array_equal(t_min, gr[key + ":t_min"]) and np.array_equal(u, gr[key + ":u"])
        assert step == float(gr[key + ":step"])
        y = r64.distortion(w, t_min, step, u)
        e = r64.errors(gr[key + ":loss"], gr[key + ":grad"], gr[key + ":per_ray"], y)
        assert max(e) <= 1e-13, (key, e)


def test_fp32_floor_reproduces_the_stored_floor(gr, gold):
    floors = r64.measure_floors(gold)
    for k, v in floors.items():
        stored = float(gr["ref32_err:" + k])
        print(f"ref32_err:{k}: measured {v:.3e}, stored {stored:.3e}, bound {r64.bound(stored):.1e}")
        assert stored / 2 <= v <= stored * 2, (k, v, stored)
        assert stored < 1e-6               # a plain fp32 implementation meets max(3 x floor, 1e-5) = 1e-5 with room


# ---- blind spots: a perturbation a broken kernel could make must move the yardstick by more than 10 x the bound, or the case proves nothing
R_GPU = 257           # max(R_ALL) of tests/test_gpu_rayregs.py: the checks below run on the first five rays of the very arrays it uploads


def _gpu_case(case, S, R=5):
    seed = r64.CASES.index(case) * 100 + S
    t_min, u, step = r64.geometry(R_GPU, S, seed)
    return r64.named_case(case, R_GPU, S, seed)[:R], t_min[:R], u[:R], step


def test_cases_do_not_depend_on_the_ray_count():
    """the first rows of a longer case are the shorter case: what the stored results, the blind-spot checks and the GPU tests share"""
    for case in r64.CASES:
        for S in (65, 129):
            for a, b in zip(_case(case, 5, S), _gpu_case(case, S)):
                assert np.array_equal(a, b), (case, S)
            assert np.array_equal(r64.named_case(case, R_GPU, S, 7)[r64.PERIOD:r64.PERIOD + 5], r64.named_case(case, 5, S, 7))


def _moves(y0, y1, gr):
    """(value, gradient) change from y0 to y1 in units of the bound"""
    e_l = abs(y1["loss"] - y0["loss"]) / abs(y0["loss"]) / r64.bound(float(gr["ref32_err:loss"]))
    e_g = r64._rel(y1["grad"], y0["grad"]) / r64.bound(float(gr["ref32_err:grad"]))
    return e_l, e_g


@pytest.mark.parametrize("case", ["two_surfaces", "fog", "zeros"])
def test_blind_spot_last_sample(gr, case):
    """S = 65, the one-lane tail chunk: the last sample zeroed.  (A spike's value does not depend on where it sits and an opaque ray's last
    weight is ~0: those two are pinned by their exact values instead.)"""
    w, t_min, u, step = _gpu_case(case, 65)
    w1 = w.copy()
    w1[:, -1] = 0.0
    m = _moves(r64.distortion(w, t_min, step, u), r64.distortion(w1, t_min, step, u), gr)
    print(case, "last sample zeroed: value %.0f x, gradient %.0f x the bound" % m)
    assert min(m) > 10.0


@pytest.mark.parametrize("case", ["two_surfaces", "fog"])
def test_blind_spot_last_ray(gr, case):
    """R = 5, the one-wave tail workgroup: the mean over four rays, and no fifth gradient row.  (The fifth ray of `zeros` is an all-zero one.)"""
    w, t_min, u, step = _gpu_case(case, 65)
    y0 = r64.distortion(w, t_min, step, u)
    y4 = r64.distortion(w[:4], t_min[:4], step, u[:4])
    y4["grad"] = np.concatenate([y4["grad"] * 4.0 / 5.0, np.zeros((1, 65))])            # rows 0..3 right, row 4 never written
    m = _moves(y0, y4, gr)
    print(case, "last ray dropped: value %.0f x, gradient %.0f x the bound" % m)
    assert min(m) > 10.0


@pytest.mark.parametrize("case", ["two_surfaces", "zeros", "opaque"])
def test_blind_spot_chunk_boundary(gr, case):
    """S = 129, the carry between the first two chunks: samples 63 / 64 swapped.  These three cases pin the carry: two_surfaces and zeros
    put a sharp surface on sample 64 of ray 0 and none on 63, an opaque ray has a 10 : 1 step there on some ray.  fog does not - its
    neighbouring weights differ by their noise only, the swap moves it by 1.9 x / 5.4 x the bounds - and is not relied on here."""
    w, t_min, u, step = _gpu_case(case, 129)
    w1 = w.copy()
    w1[:, [63, 64]] = w[:, [64, 63]]
    m = _moves(r64.distortion(w, t_min, step, u), r64.distortion(w1, t_min, step, u), gr)
    print(case, "samples 63 / 64 swapped: value %.0f x, gradient %.0f x the bound" % m)
    assert min(m) > 10.0
