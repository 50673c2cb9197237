"""CPU checks of the evaluation metrics (no GPU): the library exports the new entry points, nvfi_amd.utils.metrics / metric_segm /
point_segm_util have the reference's surface and refuse CPU tensors, the float64 yardstick (tests/metrics64.py) is pinned to the reference's own
outputs in tests/golden/metrics.npz (tests/golden/make_golden_metrics.py), and stage 2 - host numpy on the confusion matrices - reproduces every
number the reference computes from the full arrays.

Bounds.  Counts: exact.  Confidence and SSIM: the reference's own fp32 error, which the golden script measured against the yardstick and stored:
`ssim:dev` = (1.36e-07, 1.54e-07) for (ssim, cs), `segm:conf_dev` = 1.12e-07 relative; the yardstick must reproduce the goldens within exactly
those figures (they are the distance of the two, taken as the bound with a factor 1 + 1e-6 for the comparison's own rounding).
Stage 2 on the golden confusions: Pred_IoU, PQ, F1, Pre, Rec, mIoU, RI to 1e-12 (the same IEEE operations on the same integers; float32
where the reference uses float32), Pred_Matched, N_GT_Inst and AP exactly."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import metrics64 as m64
from conftest import GOLD, ROOT


@pytest.fixture(scope="module")
def mgold():
    return np.load(os.path.join(GOLD, "metrics.npz"))


def segm_case(z, name):
    pre = f"segm:{name}:"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def segm_names(z):
    return [str(n) for n in z["segm:names"]]


def ssim_names(z):
    return [str(n) for n in z["ssim:names"]]


SEGM = ["basic", "empty_pred", "zero_bg", "ignore", "multi", "two", "full8"]
SSIM_PAIRS = ["unit48", "wide", "bytes", "signed1", "smooth4"]


def test_fixture_lists(mgold):
    assert segm_names(mgold) == SEGM and ssim_names(mgold) == SSIM_PAIRS
    assert os.path.getsize(os.path.join(GOLD, "metrics.npz")) < (1 << 20)


def test_library_exports_the_metrics_entry_points():
    import ctypes as C
    from nvfi_amd import _lib
    from nvfi_amd.build import SOURCES, build
    build()
    assert "metrics.hip" in SOURCES
    L = C.CDLL(_lib.SO)
    header = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    for n in ("nvfi_metrics_workspace_bytes", "nvfi_ssim", "nvfi_segm_confusion"):
        assert hasattr(L, n) and n in _lib.EXPORTS and f"int {n}(" in header, n
    lib = _lib.lib()
    assert lib.nvfi_abi_version() == 5
    nbytes = C.c_int64(0)
    assert lib.nvfi_metrics_workspace_bytes(0, 1, 3, 800, 800, C.byref(nbytes)) == 0 and 0 < nbytes.value < (1 << 20)
    assert lib.nvfi_metrics_workspace_bytes(1, 1, 8, 0, 0, C.byref(nbytes)) == 0 and 0 < nbytes.value < (1 << 20)
    assert lib.nvfi_metrics_workspace_bytes(0, 1, 5, 800, 800, C.byref(nbytes)) != 0 and b"channels" in lib.nvfi_last_error()      # C <= 4
    assert lib.nvfi_metrics_workspace_bytes(0, 1, 3, 10, 800, C.byref(nbytes)) != 0                                                 # H, W >= 11
    assert lib.nvfi_metrics_workspace_bytes(1, 1, 33, 0, 0, C.byref(nbytes)) != 0 and b"classes" in lib.nvfi_last_error()          # K <= 32


def test_modules_have_the_reference_signatures():
    from nvfi_amd import utils
    from nvfi_amd.utils import metric_segm, metrics, point_segm_util
    want = {(metrics.SSIM.__call__, "(self, y_pred, y_true, w_size=11, size_average=True, full=False)"), (metrics.MSE.__call__, "(self, pred, gt)"),
            (metrics.PSNR.__call__, "(self, pred, gt)"), (metrics.estim_error, "(estim, gt)"), (metrics.save_error, "(errors, save_dir, ext='')"),
            (metrics.mse2psnr, "(mse)"), (metrics.ssim_frames, "(pred_hwc, gt_hwc)"),
            (metric_segm.eval_segm, "(segm, mask, ignore_npoint_thresh=0)"), (metric_segm.accumulate_eval_results, "(segm, mask, ignore_npoint_thresh=0)"),
            (metric_segm.calculate_AP, "(Pred_Matched, Confidence, N_GT_Inst, plot=False, eps=1e-10)"),
            (metric_segm.calculate_PQ_F1, "(Pred_IoU, Pred_Matched, N_GT_Inst, eps=1e-10)"),
            (metric_segm.ClusteringMetrics.__init__, "(self, spec=None)"), (metric_segm.ClusteringMetrics.forward, "(self, mask, segm, ignore_npoint_thresh=0)"),
            (point_segm_util.compress_label, "(segm)"), (point_segm_util.align_insts, "(gt_segm, segm)")}
    for fn, sig in want:
        assert str(inspect.signature(fn)) == sig, fn
    assert metric_segm.ClusteringMetrics.IOU == 1 and metric_segm.ClusteringMetrics.RI == 2
    assert list(inspect.signature(metric_segm.SegmEvaluator.__init__).parameters)[:3] == ["self", "n_object", "n_gt"]
    assert inspect.signature(utils.render_test_evaluation).parameters["with_ssim"].default is False
    for name in ("SSIM", "MSE", "PSNR", "estim_error", "save_error", "ssim_frames", "mse2psnr", "eval_segm", "accumulate_eval_results", "calculate_AP",
                 "calculate_PQ_F1", "ClusteringMetrics", "SegmEvaluator", "compress_label", "align_insts", "render_segm_evaluation"):
        assert hasattr(utils, name), name
    assert metrics.mse2psnr(0) == 50.0 and abs(metrics.mse2psnr(0.01) - 20.0) < 1e-12
    for banned in ("scipy", "matplotlib", "cv2"):
        src = "".join(open(os.path.join(ROOT, "nvfi_amd", "utils", f)).read() for f in ("metrics.py", "metric_segm.py", "point_segm_util.py"))
        assert f"import {banned}" not in src and f"from {banned}" not in src, banned


def test_kernel_stages_refuse_cpu_tensors_and_unsupported_arguments():
    from nvfi_amd._lib import NvfiError
    from nvfi_amd.utils import metric_segm, metrics
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(NvfiError):
        metrics.SSIM()(a, b)
    with pytest.raises(NvfiError):
        metrics.ssim_frames(a[0].permute(1, 2, 0), b[0].permute(1, 2, 0))
    with pytest.raises(NvfiError):
        metrics.estim_error(a, b)
    with pytest.raises(NotImplementedError):
        metrics.SSIM()(a, b, w_size=7)
    mask, segm = torch.softmax(torch.rand(1, 50, 4), -1), torch.zeros(1, 50)
    with pytest.raises(NvfiError):
        metric_segm.accumulate_eval_results(segm, mask)
    with pytest.raises(NvfiError):
        metric_segm.eval_segm(segm[0], mask[0])
    with pytest.raises(NvfiError):
        metric_segm.ClusteringMetrics()(mask, segm.long())
    with pytest.raises(NvfiError):
        metric_segm.SegmEvaluator(4).update(mask[0].reshape(5, 10, 4), segm[0].reshape(5, 10))
    with pytest.raises(NotImplementedError):
        metric_segm.calculate_AP(np.ones(2), np.array([0.5, 0.4]), 2, plot=True)


def test_metrics_source_keeps_the_rules_of_the_unit():
    """text only: no memset node (every clear is a kernel), no float atomic, nothing that waits for the device or allocates"""
    src = open(os.path.join(ROOT, "nvfi_amd", "csrc", "metrics.hip")).read()
    for word in ("hipMemset", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipMalloc", "atomicAdd(a.conf_sum", "unsafeAtomicAdd", "atomicAdd((float", "atomicAdd((double"):
        assert word not in src, word


# ---------------------------------------------------------------- the yardstick against the goldens
def test_window_is_the_reference_window(mgold):
    from nvfi_amd.utils.metrics import SSIM
    w1 = SSIM().gaussian(11, 1.5).numpy()
    assert np.array_equal(w1, mgold["ssim:window1d"])
    assert np.array_equal(SSIM().create_window(11, 3).numpy(), np.broadcast_to(mgold["ssim:window2d"], (3, 1, 11, 11)))
    # the 2-D window is the fp32 outer product of the 1-D one: the kernel's separable form differs from it by that product's rounding only
    assert np.array_equal(mgold["ssim:window2d"], np.outer(w1, w1).astype(np.float32))


@pytest.mark.parametrize("name", SSIM_PAIRS)
def test_ssim_yardstick_matches_the_reference_goldens(mgold, name):
    p, g = mgold[f"ssim:{name}:pred"], mgold[f"ssim:{name}:gt"]
    assert m64.derived_range(p) == int(mgold[f"ssim:{name}:L"])
    y = np.array(m64.ssim64(p, g, mgold["ssim:window2d"]))
    d = np.abs(y - mgold[f"ssim:{name}:ref"])
    print(f"[metrics64] {name}: ssim / cs against the fp32 golden {d[0]:.2e} / {d[1]:.2e} (stored worst case {mgold['ssim:dev']})")
    assert (d <= mgold["ssim:dev"] * (1 + 1e-6)).all()
    assert mgold["ssim:dev"].max() < 1e-6           # the fp32 reference itself is that close to float64 on these images


@pytest.mark.parametrize("name", SEGM)
def test_confusion_yardstick_matches_the_reference_goldens(mgold, name):
    from nvfi_amd.utils import metric_segm as ms
    c = segm_case(mgold, name)
    B, G, K = c["counts"].shape
    y = [m64.confusion64(c["mask"][b], c["segm"][b], G) for b in range(B)]
    for b in range(B):
        assert np.array_equal(y[b][0], c["counts"][b]) and y[b][3] == 0
        assert np.array_equal(y[b][2], c["mask"][b].argmax(1))
    conf = ms.accumulate_from_confusion([yy[0] for yy in y], [yy[1] for yy in y], int(c["thresh"]))[2]
    e = np.max(np.abs(conf - c["Confidence"]) / c["Confidence"])
    print(f"[metrics64] {name}: float64 confidences against the fp32 golden {e:.2e} (stored worst case {float(mgold['segm:conf_dev']):.2e})")
    assert e <= float(mgold["segm:conf_dev"]) * (1 + 1e-6)


# ---------------------------------------------------------------- stage 2 against the goldens
def check_summary(s, c, label=""):
    """a stage-2 summary against the golden numbers of a case: the bounds of this file, used by the GPU test as well"""
    assert np.array_equal(s["Pred_Matched"], c["Pred_Matched"]) and s["N_GT_Inst"] == int(c["N_GT_Inst"]), label
    np.testing.assert_allclose(s["Pred_IoU"], c["Pred_IoU"], rtol=1e-12, atol=0)
    AP, PQ, F1, Pre, Rec, mIoU, RI = c["scores"]
    assert s["AP"] == AP, (label, s["AP"], AP)
    for k, v in (("PQ", PQ), ("F1", F1), ("Pre", Pre), ("Rec", Rec), ("mIoU", mIoU), ("RI", RI)):
        assert abs(float(s[k]) - v) <= 1e-12 * max(abs(v), 1.0), (label, k, float(s[k]), v)


@pytest.mark.parametrize("name", SEGM)
def test_stage2_reproduces_the_reference_numbers(mgold, name):
    from nvfi_amd.utils import metric_segm as ms
    c = segm_case(mgold, name)
    thresh = int(c["thresh"])
    y = [m64.confusion64(c["mask"][b], c["segm"][b], c["counts"].shape[1])[1] for b in range(c["mask"].shape[0])]
    s = ms.summary_from_confusion(c["counts"], np.stack(y), thresh)
    check_summary(s, c, name)
    per = [ms.clustering_from_confusion(cc, None, thresh) for cc in c["counts"]]
    np.testing.assert_allclose([float(p["iou"]) for p in per], c["iou"], rtol=1e-12, atol=0)
    np.testing.assert_allclose([p["ri"] for p in per], c["ri"], rtol=1e-12, atol=0)
    # a wider ground-truth range (G = 32, the evaluator's default) changes nothing
    wide = np.zeros((c["counts"].shape[0], 32, c["counts"].shape[2]), np.int64)
    wide[:, :c["counts"].shape[1]] = c["counts"]
    check_summary(ms.summary_from_confusion(wide, np.stack(y), thresh), c, name + " G=32")


@pytest.mark.parametrize("name", SEGM)
def test_align_insts_reproduces_the_reference(mgold, name):
    from nvfi_amd.utils import point_segm_util as pu
    c = segm_case(mgold, name)
    K = c["mask"].shape[-1]
    gt_c = pu.compress_label(c["segm"].reshape(-1))
    pr_c = pu.compress_label(c["mask"].reshape(-1, K).argmax(-1))
    assert np.array_equal(pu.align_insts(gt_c, pr_c), c["aligned"])
    # and through the look-up table of the summed confusion, as SegmEvaluator does it on the device
    lut = pu.align_lut_from_confusion(c["counts"].sum(0))
    assert np.array_equal(lut[c["mask"].reshape(-1, K).argmax(-1)], c["aligned"])


def test_assignment_solver_equals_brute_force():
    from nvfi_amd.utils.metric_segm import linear_assignment
    rng = np.random.default_rng(11)
    for trial in range(120):
        r, c = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        v = rng.random((r, c)) if trial % 3 else np.round(rng.random((r, c)) * 4) / 4          # (every third: many ties and zeros)
        for maximize in (True, False):
            ri, ci = linear_assignment(v, maximize)
            assert len(ri) == min(r, c) and len(set(ci.tolist())) == len(ci) and (np.diff(ri) > 0).all()
            got = v[ri, ci].sum()
            a = v if r <= c else v.T
            sums = [a[np.arange(a.shape[0]), list(p)].sum() for p in itertools.permutations(range(a.shape[1]), a.shape[0])]
            want = max(sums) if maximize else min(sums)
            assert abs(got - want) <= 1e-12, (trial, r, c, maximize, got, want)


def test_rand_index_from_confusion_equals_the_pairwise_form():
    from nvfi_amd.utils.metric_segm import clustering_from_confusion, rand_index_counts
    rng = np.random.default_rng(5)
    for N, G, K in ((1, 1, 1), (37, 3, 4), (300, 6, 2), (513, 8, 8)):
        a, b = rng.integers(0, G, N), rng.integers(0, K, N)
        counts = np.zeros((G, K), np.int64)
        np.add.at(counts, (a, b), 1)
        agree = int(((a[:, None] == a[None, :]) == (b[:, None] == b[None, :])).sum())
        assert rand_index_counts(counts) == (agree, N * N)
        assert clustering_from_confusion(counts, [2])["ri"] == float(np.float32(agree) / np.float32(N * N))
    # restricted to the points of large enough objects
    a = np.array([0] * 40 + [1] * 30 + [2] * 3)
    b = rng.integers(0, 3, a.size)
    counts = np.zeros((3, 3), np.int64)
    np.add.at(counts, (a, b), 1)
    keep = a != 2
    agree = int(((a[keep][:, None] == a[keep][None, :]) == (b[keep][:, None] == b[keep][None, :])).sum())
    assert clustering_from_confusion(counts, [2], ignore_npoint_thresh=10)["ri"] == float(np.float32(agree) / np.float32(70 * 70))
    # at frame size the count stays an exact integer
    big = np.array([[400000, 1000], [2000, 237000]], np.int64)
    agree, pairs = rand_index_counts(big)
    assert pairs == 640000 ** 2 and agree == pairs - (401000 ** 2 + 239000 ** 2) - (402000 ** 2 + 238000 ** 2) + 2 * (400000 ** 2 + 1000 ** 2 + 2000 ** 2 + 237000 ** 2)
