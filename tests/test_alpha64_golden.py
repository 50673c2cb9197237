"""The float64 restatement of the occupancy path (tests/alpha64.py, and render64's `alpha_volume`) against the reference's own outputs that are
already under tests/golden/: this pins the yardstick that tests/test_gpu_alpha64.py holds the device to.

  hotpath.npz  {A,B}:amask:pts / amask:alpha       sample_alpha64 on 300 points of [-1.1, 1.1]^3 (83 / 73 of them outside the volume: zero padding)
               {A,B}:render_amask:*                render64(..., alpha_volume=volume): rgb, depth, acc, weight of the eval render through the mask
  r2.npz       {As,Bs}:dense_alpha, As:dense_alpha_transfer, {As,Bs}:mask_volume, {As,Bs}:new_aabb

Measured (CPU, torch 2.10).  The goldens are fp32 outputs of the reference; the float32 evaluation of the yardstick reproduces them to the printed
digits, so what is left is fp32 rounding in both columns:
                          float64 against the golden          float32 evaluation against float64      bound (3 x the worst, rounded up)
  sample_alpha            1.1e-7 (A), 1.3e-7 (B) abs          1.1e-7, 1.3e-7                          4e-7 absolute (values in [0, 1])
  render_amask maps       rgb 2.0e-7, depth 1.8e-6,           rgb 1.5e-7, depth 1.4e-6,               the sibling file's: rtol 4e-6 +
                          acc 2.5e-7, weight 8.3e-7 abs       acc 2.7e-7, weight 9.4e-7               helpers.FP32_FLOOR (nothing leaves the floor)
  dense_alpha (floors())  As 4.3e-8 / 3.9e-6, As transfer     the same, As transfer 6.5e-8 / 7.3e-6   DENSE_ATOL 2.1e-7, DENSE_RTOL 2.3e-5
                          5.0e-8 / 7.4e-6, Bs 6.7e-8 / 7.5e-6
  alpha near the mask threshold (within a decade of 1e-4): 3.3e-8 absolute on all three -> MASK_DELTA 1e-7
Mask volumes: 0 voxels differ from the golden on As and on Bs; voxels with a margin below MASK_DELTA: As 0 of 5 760, Bs 2 of 4 896 (0.04 %; the
limit asserted is 0.1 %).  new_aabb is bit-equal.  The golden `amask` volume itself culls next to nothing (A: 0, B: 37 of 9 651 in-box samples):
the volumes that do cull are those of tests/test_gpu_alpha64.py, whose yardstick-only conditions (near-face points, culled fractions) are
asserted here on the CPU as well.

The element-wise compute_alpha cases of the GPU file (alpha64.alpha_cases x alpha64.SIZES on fields A and B): the float32 floors are measured
again here and 3 x each must stay under alpha64.ALPHA_ATOL / ALPHA_RTOL (the table is in alpha64.py); points within 4 fp32 ulp of a gate face:
none at any size (limit 0.5 %); the step counts are 0 / 1 / 1 / 2 / 8 on field A and 0 / 1 / 1 / 8 / 40 on field B.  The frame times i / 60 at which
fp32(i / 60) is isclose to a keyframe without being equal to it (where nvfi_compute_alpha used to skip the reference's step): none on As, 27/60
and 39/60 on Bs (2 of 60 times, every in-gate voxel, a step of 3e-8)."""
import os

import numpy as np
import pytest
import torch

import alpha64 as a64
import render64 as r64
from conftest import GOLD
from helpers import FP32_FLOOR, load_meta
from test_render64_golden import MAP_RTOL, fields64      # noqa: F401  (the fixture and the eval-map bound of the sibling file)

KINDS = ["A", "B"]
SAMPLE_ATOL = 4e-7
NEAR_MAX = 1e-3


@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(GOLD, "r2.npz"))


@pytest.mark.parametrize("kind", KINDS)
def test_sample_alpha64_matches_the_reference_golden(gold, kind):
    vol, pts, ref = gold[f"{kind}:render_amask:volume"], gold[f"{kind}:amask:pts"], gold[f"{kind}:amask:alpha"].astype(np.float64)
    a, ulps, near = a64.sample_alpha64(vol, pts)
    a32, _, _ = a64.sample_alpha64(vol, pts, torch.float32)
    outside = (np.abs(pts) > 1).any(1)
    print(f"[alpha64] {kind}:amask: max abs err against the golden {np.abs(a - ref).max():.2e}, float32 evaluation against float64 "
          f"{np.abs(a32 - a).max():.2e}; {int(outside.sum())} points outside the volume, {int((ref[outside] > 0).sum())} of them read a border voxel; "
          f"{int(near.sum())} near a voxel boundary")
    assert outside.sum() > 50 and (ref[outside] > 0).any() and (ref[outside] == 0).any()
    assert np.abs(a - ref).max() <= SAMPLE_ATOL
    assert np.array_equal(a > 0, ref > 0) or near.any()
    assert np.array_equal(np.floor(a64.voxel_coord(pts, vol.shape[::-1])), np.floor(a64.voxel_coord_device(pts, vol.shape[::-1])))


@pytest.mark.parametrize("kind", KINDS)
def test_render64_matches_the_reference_amask_golden(gold, fields64, kind):
    f, meta = fields64[kind]
    pre = f"{kind}:render_amask:"
    o, d = gold[f"{kind}:rays_o"], gold[f"{kind}:rays_d"]
    wb = bool(meta["white_background"])
    kw = dict(loss=None, grads=False, alpha_volume=gold[pre + "volume"])
    r = r64.render64(f, o, d, 19.0 / 60.0, None, wb, **kw)
    r32 = r64.render64(f, o, d, 19.0 / 60.0, None, wb, dtype=torch.float32, **kw)
    print(f"[alpha64] {pre} {int(r['culled'].sum())} of {int(r['in_box'].sum())} in-box samples culled, {int(r['alpha_near'].sum())} near a voxel boundary")
    assert np.array_equal(r["culled"], r32["culled"]) and not r["alpha_near"].any()
    for m in ("rgb", "depth", "acc", "weight"):
        ref = gold[pre + m].astype(np.float64)
        err = np.abs(r[m] - ref)
        print(f"[alpha64] {pre}{m}: max abs err {err.max():.2e}, float32 evaluation against float64 {np.abs(r32[m] - r[m]).max():.2e}")
        assert (err <= MAP_RTOL * np.abs(ref) + FP32_FLOOR[m]).all(), (pre, m, float(err.max()))
    # a train-mode call (a jitter is given) does not cull
    rt = r64.render64(f, o, d, 19.0 / 60.0, np.zeros(len(o), np.float32), wb, **kw)
    assert "culled" not in rt and rt["valid"].sum() == r["in_box"].sum()


@pytest.mark.parametrize("kind", KINDS)
def test_dense_alpha64_and_mask_match_the_reference_goldens(g2, kind):
    meta, _ = load_meta(kind)
    f = a64.field_from_npz(g2, f"{kind}s:", meta)
    pre = f"{kind}s:"
    gs = [int(g) for g in g2[pre + "gridSize"]]
    thres = float(meta["alphaMask_thres"])
    for transfer in ([False, True] if kind == "A" else [False]):
        ref = g2[pre + ("dense_alpha_transfer" if transfer else "dense_alpha")].astype(np.float64)
        d = a64.dense_alpha64(f, gs, transfer)
        d32 = a64.dense_alpha64(f, gs, transfer, torch.float32)
        ga, gr = a64.floors(ref, d["alpha"])
        fa, fr = a64.floors(d32["alpha"], d["alpha"])
        band = (d["alpha"] > thres / 10) & (d["alpha"] < thres * 10)
        at = np.abs(d32["alpha"] - d["alpha"])[band].max()
        print(f"[alpha64] {pre}dense_alpha{'_transfer' if transfer else ''}: float64 against the golden abs {ga:.2e} rel {gr:.2e}; float32 evaluation "
              f"against float64 abs {fa:.2e} rel {fr:.2e}; within a decade of the threshold ({int(band.sum())} voxels) {at:.2e}; near a gate face "
              f"{int(d['edge'].sum())} voxels; keyframe-shortcut times {d['shortcut_times']}")
        assert ref.shape == d["alpha"].shape
        assert (np.abs(d["alpha"] - ref) <= a64.DENSE_RTOL * np.abs(ref) + a64.DENSE_ATOL).all(), (ga, gr)
        assert 3 * fa <= a64.DENSE_ATOL and 3 * fr <= a64.DENSE_RTOL and 3 * at <= a64.MASK_DELTA, (fa, fr, at)
        if transfer:
            continue
        m = a64.update_alpha_mask64(d["alpha"], d["xyz"], thres)
        vref = g2[pre + "mask_volume"][0, 0]
        near = m["margin"] < a64.MASK_DELTA
        diff = m["volume"] != vref
        print(f"[alpha64] {pre}mask_volume: {int(diff.sum())} voxels differ from the golden, {int(near.sum())} of {near.size} lie within "
              f"{a64.MASK_DELTA:g} of the threshold; smallest margin {m['margin'].min():.2e}; {vref.mean():.3f} of the volume is set")
        assert m["volume"].shape == vref.shape and not (diff & ~near).any()
        assert near.sum() <= NEAR_MAX * near.size
        assert np.array_equal(m["new_aabb"], g2[pre + "new_aabb"]) or a64.aabb_near(m["volume"], near, d["xyz"])


@pytest.mark.parametrize("kind", KINDS)
def test_compute_alpha_cases_floors_and_near_face_points(fields64, kind):
    """the yardstick-only conditions of the GPU file's element-wise cases: the float32 floors under a third of the bounds, the near-face points
    at most 0.5 % of a case, the step counts"""
    f, _ = fields64[kind]
    steps = []
    for label, t, transfer, nsteps, every in a64.alpha_cases(f):
        wa = wr = 0.0
        for N in a64.SIZES:
            if N > a64.MULTI_STEP_MAX_N and not every:
                continue
            x = a64.case_points(f, N)
            r = a64.compute_alpha64(f, x, t, transfer)
            r32 = a64.compute_alpha64(f, x, t, transfer, dtype=torch.float32)
            assert len(r["steps"]) == nsteps and r["shortcut"] == (label == "nearkey"), (label, len(r["steps"]))
            edge = r["edge"] | r32["edge"]
            assert edge.sum() <= int(0.005 * N), (kind, label, N, int(edge.sum()))
            fa, fr = a64.floors(r32["alpha"][~edge], r["alpha"][~edge])
            wa, wr = max(wa, fa), max(wr, fr)
            if N >= 31:
                xn = a64.normalize32(f, x).numpy()
                assert (np.abs(xn) > 1).any() and (np.abs(xn[:9]) >= 1 - 1e-6).any(1).all(), "points beyond the box, and on its faces"
        steps.append(nsteps)
        print(f"[alpha64] {kind}:{label}: {nsteps} steps, float32 floor abs {wa:.2e} rel {wr:.2e} (bounds {a64.ALPHA_ATOL:g} / {a64.ALPHA_RTOL[kind][label]:g})")
        assert 3 * wa <= a64.ALPHA_ATOL and 3 * wr <= a64.ALPHA_RTOL[kind][label], (kind, label, wa, wr)
    assert steps == ([0, 1, 1, 2, 8] if kind == "A" else [0, 1, 1, 8, 40]), steps


def test_block_volume_culls_and_near_reporting():
    """the synthetic volume of the GPU file: three different extents, half of it set; and sample_alpha64's near flag on constructed points: a
    point exactly on a voxel plane between an empty and a set block is near, a point in the middle of a voxel is not"""
    vol = a64.block_volume()
    assert vol.shape == (41, 50, 37) and 0.4 < vol.mean() < 0.6
    W, H, D = 37, 50, 41
    # voxel (x, y, z) = (5, 3, 2) is empty with an empty neighbourhood below x = 6; x = 6 starts a set block
    assert vol[2, 3, 5] == 0 and vol[2, 3, 6] == 1 and vol[2, 3, 4] == 0
    def xn(ix, size):
        return np.float32(2.0 * ix / (size - 1) - 1.0)
    on_plane = np.array([[xn(5, W), xn(3.5, H), xn(2.5, D)]], np.float32)
    mid = np.array([[xn(4.5, W), xn(3.5, H), xn(2.5, D)]], np.float32)
    a, ulps, near = a64.sample_alpha64(vol, np.concatenate([on_plane, mid]))
    assert ulps[0, 0] <= a64.NEAR_ULP and near[0] and not near[1] and a[1] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_dense_end_to_end_bounds_cover_the_float32_floor(g2, kind):
    """the bounds of the GPU file's end-to-end cases on the small grid (the 33 x 31 x 29 figures are recorded in alpha64.py): 3 x the float32 floor
    stays under them, and under MASK_DELTA at the threshold"""
    meta, _ = load_meta(kind)
    f = a64.field_from_npz(g2, f"{kind}s:", meta)
    thres = float(meta["alphaMask_thres"])
    for transfer in (False, True):
        d = a64.dense_alpha64(f, (7, 5, 9), transfer)
        d32 = a64.dense_alpha64(f, (7, 5, 9), transfer, torch.float32)
        k = ~(d["edge"] | d32["edge"])
        fa, fr = a64.floors(d32["alpha"][k], d["alpha"][k])
        band = (d["alpha"] > thres / 10) & (d["alpha"] < thres * 10)
        at = np.abs(d32["alpha"] - d["alpha"])[band].max() if band.any() else 0.0
        rtol, atol = a64.DENSE_E2E[(kind, 7, transfer)]
        print(f"[alpha64] {kind}s 7x5x9 {'transfer' if transfer else 'plain'}: float32 floor abs {fa:.2e} rel {fr:.2e} (bounds {atol:g} / {rtol:g}), at the threshold {at:.2e}")
        assert 3 * fa <= atol and 3 * fr <= rtol and 3 * at <= a64.MASK_DELTA, (fa, fr, at)
