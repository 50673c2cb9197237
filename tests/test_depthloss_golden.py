"""Depth loss, CPU side: the float64 yardstick (tests/depth64.py) against goldens made with the reference's own compute_depth_loss
(tests/golden/make_golden_depth.py), its holes / gather arguments against plain numpy subsets, and the presence of the feature at every layer
(ABI, binding, utils)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth64 as d64
from conftest import GOLD, ROOT
from nvfi_amd._lib import NVFI_DEPTH_LDS_MAX, NVFI_DEPTH_SKIP_HOLES      # the module is the CPU side of the feature: without the binding nothing here runs

SIZES = (1, 2, 3, 64, 65, 2048)
CASES = ("distinct", "plateau", "allequal", "signed")


@pytest.fixture(scope="module")
def gd():
    return np.load(os.path.join(GOLD, "depthloss.npz"))


@pytest.mark.parametrize("case", CASES)
def test_depth64_reproduces_reference_goldens(gd, case):
    """bound: the reference's own fp32 error against the yardstick, stored beside the goldens (absolute for the loss, relative to
    depth64.grad_scale for the gradient: max|grad|, except on the two n = 2 cases whose gradient is a cancellation of its own terms - with them
    measured against max|grad| the figure was 1.2e-2 and bounded nothing); an exact zero (n = 1) is an exact zero"""
    tol_l, tol_g = float(gd["ref32_err:loss"]), float(gd["ref32_err:grad"])
    for n in SIZES:
        key = f"{case}:{n}"
        pred, gt = gd[key + ":pred"], gd[key + ":gt"]
        assert pred.dtype == np.float32 and pred.shape == (n,)
        y = d64.depth64(pred, gt)
        e_l, e_g = d64.errors(gd[key + ":loss"], gd[key + ":grad"], y)
        print(f"{key}: loss err {e_l:.2e} (bound {tol_l:.2e}), grad err {e_g:.2e} (bound {tol_g:.2e})")
        assert e_l <= tol_l and e_g <= tol_g, (key, e_l, e_g)
        assert y["n_counted"] == n
        assert (d64.grad_scale(y) != np.abs(y["grad"]).max()) == (key in ("distinct:2", "plateau:2")), key      # the ill-conditioned cases, by name
        if n == 1:
            assert y["loss"] == 0.0 and not y["grad"].any() and float(gd[key + ":loss"]) == 0.0 and not gd[key + ":grad"].any()


def test_plateau_splits_the_median_gradient_equally(gd):
    """60 % of pred equal far: the median is far, and every tied entry with the same target term gets the same share.  The reference's
    gradient (torch autograd) shows the split: perturbing which tied entry a sort would pick changes nothing."""
    pred, gt = gd["plateau:2048:pred"], gd["plateau:2048:gt"]
    y = d64.depth64(pred, gt)
    tie = pred == np.float32(8.0)
    assert y["med_pred"] == 8.0 and tie.sum() >= 1024
    # the part of the gradient that does not come from a_j / (s + eps) is the same for every tied entry
    nc = pred.size
    inv_p = 1.0 / (np.mean(np.abs(pred.astype(np.float64) - 8.0)) + d64.EPS)
    gtd = gt.astype(np.float64)
    inv_g = 1.0 / (np.mean(np.abs(gtd - d64.lower_median(gtd))) + d64.EPS)
    a = 2.0 * ((pred.astype(np.float64) - 8.0) * inv_p - (gtd - d64.lower_median(gtd)) * inv_g) / nc
    rest = y["grad"] - a * inv_p
    assert np.ptp(rest[tie]) <= 1e-12 * np.abs(rest[tie]).max()
    ref_rest = gd["plateau:2048:grad"].astype(np.float64) - a * inv_p
    assert np.ptp(ref_rest[tie]) <= 4 * float(gd["ref32_err:grad"]) * np.abs(y["grad"]).max()
    # [5,2,2,2,1]: thirds
    g = d64.depth64(np.array([5, 2, 2, 2, 1], np.float32), np.array([1, 2, 3, 4, 5], np.float32))
    assert g["med_pred"] == 2.0


def test_signed_case_has_both_zeros_and_they_tie(gd):
    pred = gd["signed:2048:pred"]
    z = pred == 0
    assert np.signbit(pred[z]).any() and (~np.signbit(pred[z])).any() and (pred < 0).any()
    y = d64.depth64(pred, gd["signed:2048:gt"])
    assert y["med_pred"] == 0.0
    rest_neg, rest_pos = y["grad"][z & np.signbit(pred)], y["grad"][z & ~np.signbit(pred)]
    assert rest_neg.size and rest_pos.size


@pytest.mark.parametrize("n", [3, 65, 2048])
def test_holes_and_gather_equal_plain_subsets(n):
    rng = np.random.default_rng(31 + n)
    pred, gt = d64.named_case("plateau", n, 77 + n)
    # holes: 0, -1, inf, NaN at a seeded third of the entries
    gt_h = gt.copy()
    holes = rng.permutation(n)[: n // 3]
    gt_h[holes] = np.array([0.0, -1.0, np.inf, np.nan], np.float32)[np.arange(len(holes)) % 4]
    m = d64.counted_mask(gt_h, True)
    assert m.sum() == n - len(holes)
    full, sub = d64.depth64(pred, gt_h, skip_holes=True), d64.depth64(pred[m], gt_h[m])
    assert full["loss"] == sub["loss"] and full["n_counted"] == int(m.sum())
    assert np.array_equal(full["grad"][m], sub["grad"]) and not full["grad"][~m].any()
    # gather: repeated and permuted indices into a longer image
    image = rng.uniform(1.0, 8.0, 3 * n + 5).astype(np.float32)
    index = rng.integers(0, image.size, n)
    index[: n // 2] = rng.permutation(index[: n // 2])
    if n > 2:
        index[1] = index[0]
    a, b = d64.depth64(pred, image, gt_index=index), d64.depth64(pred, image[index])
    assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"])
    # all holes
    z = d64.depth64(pred, np.zeros(n, np.float32), skip_holes=True)
    assert z["loss"] == 0.0 and z["n_counted"] == 0 and not z["grad"].any()


def test_yardstick_gradient_is_the_derivative():
    """central differences of the float64 loss away from the kink of |.| and from the median's ties"""
    rng = np.random.default_rng(5)
    pred, gt = rng.uniform(1, 8, 33), rng.uniform(1, 8, 33)
    y = d64.depth64(pred, gt)
    h = 1e-6
    for j in range(33):
        e = np.zeros(33)
        e[j] = h
        fd = (d64.depth64(pred + e, gt)["loss"] - d64.depth64(pred - e, gt)["loss"]) / (2 * h)
        assert abs(fd - y["grad"][j]) <= 1e-6 * np.abs(y["grad"]).max(), (j, fd, y["grad"][j])


def test_e2e_golden_is_consistent(gd):
    """the stored upstream gradient of the depth map is w x the yardstick's gradient at the stored depth, the median is isolated"""
    depth, gt, w = gd["e2e:depth"], gd["e2e:gt"], float(gd["e2e:w"])
    subset = gd["e2e:subset"]
    assert np.array_equal(np.nonzero(gt > 0)[0], subset)
    y = d64.depth64(depth, gt, skip_holes=True)
    e_l, e_g = d64.errors(gd["e2e:loss_depth"], gd["e2e:g_depth"].astype(np.float64) / w, y)
    assert e_l <= 4 * max(float(gd["ref32_err:loss"]), 2.0 ** -23 * y["loss"]) and e_g <= 4 * max(float(gd["ref32_err:grad"]), 2.0 ** -23)
    d = np.sort(depth[subset].astype(np.float64))
    k = (d.size - 1) // 2
    need = 10 * (1e-4 * abs(d[k]) + 2e-5)
    assert d[k] - d[k - 1] >= need and d[k + 1] - d[k] >= need


def test_exports_constants_and_header():
    from nvfi_amd import _lib
    from nvfi_amd.build import SOURCES
    assert "depthloss.hip" in SOURCES and "nvfi_depth_loss" in _lib.EXPORTS
    assert os.path.exists(_lib.SO), "libnvfi_hip.so has not been built"
    L = ctypes.CDLL(_lib.SO)
    assert hasattr(L, "nvfi_depth_loss") and L.nvfi_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert "int nvfi_depth_loss(" in header
    assert int(re.search(r"#define NVFI_DEPTH_LDS_MAX (\d+)", header).group(1)) == NVFI_DEPTH_LDS_MAX
    assert int(re.search(r"#define NVFI_DEPTH_SKIP_HOLES (\d+)", header).group(1)) == NVFI_DEPTH_SKIP_HOLES


def test_python_surface_refuses_the_cpu_and_a_target_gradient():
    import inspect
    from nvfi_amd import _lib, utils
    from nvfi_amd.models.tensorf_keyframe import TensorVMKeyframeTimeKplane
    from nvfi_amd.utils.evaluation_utils import compute_depth_loss, render_test_evaluation
    assert utils.compute_depth_loss is compute_depth_loss
    assert list(inspect.signature(compute_depth_loss).parameters)[:2] == ["pred", "gt"]
    sig = inspect.signature(TensorVMKeyframeTimeKplane.render_mse_backward_).parameters
    assert sig["target_depth"].default is None and sig["depth_index"].default is None and sig["depth_weight"].default == 1.0 and sig["skip_holes"].default is False
    assert inspect.signature(render_test_evaluation).parameters["gt_depths"].default is None
    with pytest.raises(_lib.NvfiError):
        compute_depth_loss(torch.rand(8), torch.rand(8))
    with pytest.raises(NotImplementedError):
        compute_depth_loss(torch.rand(8), torch.rand(8).requires_grad_(True))
    assert not hasattr(utils, "depth_loss_raw")            # the thin binding stays in utils.evaluation_utils
