"""f-3 grid maintenance against REFERENCE goldens (tests/golden/make_golden_r2.py; reference models/tensorf_keyframe.py:327-499):
getDenseAlpha over all 60 frame times (plain and transfer), updateAlphaMask (mask volume + returned box), shrink (cropped planes,
corrected box, step size, sample count, and an eval render of the shrunk field through its alpha mask) and upsample_volume_grid
(all 12 planes, keyframe count change, render).  Fields: "As" bat-like (VelocityAABB, K = 4) with a tight blob that really shrinks;
"Bs" chessboard-like (VelocityAABBSur, K = 16) with culled space but a box that stays (the clamp branch of shrink)."""
import os

import numpy as np
import pytest
import torch

import alpha64 as a64
import render64 as r64
from conftest import GOLD
from helpers import make_model, assert_contract, field_state
from test_gpu_alpha64 import mask_flips_only_near

pytestmark = pytest.mark.gpu
PLANES = ("density_plane_space", "density_plane_time", "app_plane_space", "app_plane_time")


@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(GOLD, "r2.npz"))


def _model(g2, kind):
    model, meta = make_model(kind)            # config of field A / B ...
    own = model.state_dict()
    pre = f"{kind}s:sd:"
    n = 0
    for k in g2.files:                        # ... with the tight-blob parameters of the r2 fixture
        if k.startswith(pre) and k[len(pre):] in own:
            own[k[len(pre):]].copy_(torch.from_numpy(np.ascontiguousarray(g2[k])).cuda())
            n += 1
    assert n >= 40
    model.nvfi._fix_layout()
    return model, meta


def _rays(kind):
    z = np.load(os.path.join(GOLD, "hotpath.npz"))
    return torch.from_numpy(z[f"{kind}:rays_o"]).cuda(), torch.from_numpy(z[f"{kind}:rays_d"]).cuda()


@pytest.mark.parametrize("kind", ["A", "B"])
def test_grid_maintenance_matches_reference(g2, kind):
    from nvfi_amd.models import Renderer, Ray
    model, meta = _model(g2, kind)
    f = model.nvfi
    f.eval()
    pre = f"{kind}s:"
    gs = [int(g) for g in g2[pre + "gridSize"]]
    # ---- getDenseAlpha: running maximum over the 60 frame times i/60 (tensorf_keyframe.py:461-499)
    alpha, dense = f.getDenseAlpha(gs)
    ref = g2[pre + "dense_alpha"]
    np.testing.assert_allclose(alpha.cpu().numpy(), ref, rtol=2e-4, atol=2e-6)
    if kind == "A":
        alpha_t, _ = f.getDenseAlpha(gs, transfer=True)
        np.testing.assert_allclose(alpha_t.cpu().numpy(), g2[pre + "dense_alpha_transfer"], rtol=2e-4, atol=2e-6)
    # ---- updateAlphaMask (:379-405)
    fld = r64.Field(*field_state(model))
    d64 = a64.dense_alpha64(fld, gs, device="cuda")               # the float64 yardstick (tests/alpha64.py) says which voxels sit at the threshold
    new_aabb = f.updateAlphaMask(gs)
    vol, vref = f.alphaMask.alpha_volume.cpu().numpy(), g2[pre + "mask_volume"]
    assert vol.shape == vref.shape
    assert np.mean(vol != vref) < 1e-3, np.mean(vol != vref)
    # a voxel may flip only where the yardstick's dilated alpha lies within MASK_DELTA of the 1e-4 threshold - against the yardstick and the golden
    m64, near = mask_flips_only_near(vol, d64["alpha"], d64["xyz"], float(meta["alphaMask_thres"]), f"{kind}s grid maintenance")
    assert not ((vol[0, 0] != vref[0, 0]) & ~near).any(), "a mask voxel differs from the golden away from the threshold"
    assert 0.05 < vref.mean() < 0.95                               # the fixture has both culled and kept space
    np.testing.assert_allclose(new_aabb.cpu().numpy(), g2[pre + "new_aabb"], rtol=1e-6, atol=1e-6)
    # ---- shrink (:407-458)
    before = {nm: [p.detach().clone() for p in getattr(f, nm)] for nm in PLANES}
    f.shrink(new_aabb)
    assert f.gridSize.tolist() == [int(g) for g in g2[pre + "shrink:gridSize"]]
    np.testing.assert_allclose(f.aabb.cpu().numpy(), g2[pre + "shrink:aabb"], rtol=1e-6, atol=1e-6)
    assert abs(float(f.stepSize) - float(g2[pre + "shrink:stepSize"])) <= 1e-6 * float(g2[pre + "shrink:stepSize"])
    assert f.nSamples == int(g2[pre + "shrink:nSamples"])
    for nm in PLANES:
        for i in range(3):
            p = getattr(f, nm)[i]
            assert p.is_contiguous(memory_format=torch.channels_last)
            assert np.array_equal(p.detach().cpu().numpy(), g2[pre + f"shrink:{nm}.{i}"]), (nm, i)      # a crop: bit-exact
    if kind == "A":
        assert f.gridSize.tolist() != gs and before["density_plane_space"][0].shape != f.density_plane_space[0].shape
    o, d = _rays(kind)
    wb = bool(meta["white_background"])
    ren = Renderer(model, 0, 0, 2048)
    out = ren.render(19.0 / 60.0, Ray(o, d, 0, 1), white_background=wb, mode="test")      # shrunk box + alpha-mask culling
    for i, nm in enumerate(("rgb", "depth", "acc")):
        assert_contract(out[i].cpu().numpy(), g2[pre + f"shrink:render:{nm}"], nm, label=f"hip {kind}s shrink")
    # ---- upsample_volume_grid (:327-376): bilinear align_corners resampling of all 12 planes, K 4 -> 6 for the bat-like field
    tgt, newK = [int(g) for g in g2[pre + "up:target"]], int(g2[pre + "up:K"])
    f.upsample_volume_grid(tgt, newK)
    assert f.gridSize.tolist() == tgt and f.num_keyframes == newK
    assert abs(float(f.stepSize) - float(g2[pre + "up:stepSize"])) <= 1e-6 * float(g2[pre + "up:stepSize"])
    assert f.nSamples == int(g2[pre + "up:nSamples"])
    for nm in PLANES:
        for i in range(3):
            p = getattr(f, nm)[i]
            assert p.is_contiguous(memory_format=torch.channels_last)
            np.testing.assert_allclose(p.detach().cpu().numpy(), g2[pre + f"up:{nm}.{i}"], rtol=1e-5, atol=1e-6, err_msg=f"{nm}.{i}")
    f.alphaMask = None
    out = ren.render(19.0 / 60.0, Ray(o, d, 0, 1), white_background=wb, mode="test")
    for i, nm in enumerate(("rgb", "depth", "acc")):
        assert_contract(out[i].cpu().numpy(), g2[pre + f"up:render:{nm}"], nm, label=f"hip {kind}s upsample")


def test_dense_alpha_at_shipped_size():
    """updateAlphaMask at the reference's default 200^3 grid (8e6 points per frame time; train_nvfi.py:337,413 call sites) on the
    bat 199^3 field: the workspace comes from nvfi_alpha_workspace_bytes (a hard-coded size failed above ~17k points)."""
    import bench
    model = bench.build_scene(torch.device("cuda", 0), 199, 128, True)
    f = model.nvfi
    f.eval()
    new_aabb = f.updateAlphaMask((200, 200, 200))
    v = f.alphaMask.alpha_volume
    assert tuple(v.shape[-3:]) == (200, 200, 200) and 0.0 < float(v.mean()) < 1.0
    assert (new_aabb[0] >= f.aabb[0] - 1e-5).all() and (new_aabb[1] <= f.aabb[1] + 1e-5).all() and (new_aabb[1] > new_aabb[0]).all()
    # the blob is centred: the mask must keep the centre voxel and cull the corner
    assert float(v[0, 0, 100, 100, 100]) == 1.0 and float(v[0, 0, 0, 0, 0]) == 0.0
