"""The occupancy path on the device - nvfi_compute_alpha (csrc/abi.hip), field.getDenseAlpha / updateAlphaMask built on it, and alpha_lookup
(csrc/render_rays.hip), the read that decides `valid` for every sample of an eval render once a mask exists - against its float64 restatement
(tests/alpha64.py and render64's alpha_volume, pinned to the reference's goldens by tests/test_alpha64_golden.py).  The float64 references run in
torch on the GPU.

(a) test_compute_alpha_elementwise: fields A (VelocityAABB) and B (VelocityAABBSur, step rejection), N in alpha64.SIZES (the 32-point wave tile, the
    128-point workgroup, the 256-thread prep / finish blocks, the 32-point blocks of k_density_q, one point over 2^15), world points over 1.15 x the
    box with nine of them on faces, edges and corners, the times of alpha64.alpha_cases (keyframe: no step; 19/60: one; 0.93: 2 / 8; 59/60 with
    transfer: 8 steps on field A (K = 4, tmax = 0.75, dt_max = 0.125) and 40 on field B (K = 16, dt_max = 0.025), asserted from the schedule - these
    two at N <= 257; and a time isclose to a keyframe, where the reference takes a tiny step that the call used to skip), both integrators
    (the default x6 and vel_fp16 bit 3, the fp32 MFMA kernels), both store modes: accumulate_max = 0 into a buffer of sentinels, accumulate_max = 1
    into a buffer prefilled below, at and above the plain result (expected: max(prefill, alpha64), and bit for bit max(prefill, plain result)).
    Bound per element |got - ref| <= rtol |ref| + atol with alpha64.ALPHA_RTOL / ALPHA_ATOL: 3 x the float32 evaluation of the yardstick on the same
    case (CPU), 25 - 100 x under the rtol 2e-4 and 12 x under the atol 2e-6 of the older tests.  No point of these inputs lies within 4 ulp of a gate
    face (asserted on the CPU, limit 0.5 %); such a point would be compared apart (finite, in [0, 1]) and every other point has no allowance.
    The published size: the workspace carries a 4 KiB tail of 0xA5 behind nvfi_alpha_workspace_bytes(N), the call is given exactly the published
    count and the tail must be untouched; with 256 bytes less the call returns 4 and neither the output nor ANY byte of the workspace changes.
(b) test_alpha_mask_culling: volumes that cull between 20 % and 80 % of the in-box samples of the golden rays (asserted from the yardstick alone):
    the real mask of As on its own 20 x 18 x 16 grid (58 %), of Bs on 33 x 31 x 29 (35 %; on its own 16 x 17 x 18 grid the dilated mask culls 5 %),
    a block pattern of 37 x 50 x 41 on field A (30 %), and the mask of As built on 10 x 9 x 8 and then read STALE after shrink() in the new box's
    coordinates (55 %; built on 20 x 18 x 16 it culls 80.03 %).  R in {1, 3, 4, 5, 257} golden rays (k_sample takes four per block; the 257th is ray
    0 again) at 19/60 and at the keyframe 0.25.  last_counters[0] equals the yardstick's valid count exactly (no sample of these renders sits on a
    voxel boundary; the limit is 0.5 % of the rays); rgb, depth, acc, weight within test_gpu_render64's MAP_RTOL x |ref| + FP32_FLOOR on the
    device's own appearance mask.  Sensitivity: inverting the yardstick's culling decision for the last in-box sample of the last ray moves a map of
    that ray beyond its bound (field A's density floor gives every in-box sample a weight of 1.3e-4); a volume where no case sees it must be listed
    in BLIND and is asserted to be blind.  The voxel coordinate in alpha_lookup's order of operations and in ATen's: the floors are counted.
(c) test_dense_alpha_and_mask_end_to_end: getDenseAlpha / updateAlphaMask on As and Bs at 7 x 5 x 9 and 33 x 31 x 29 (transfer on the small grid):
    the alpha volume element-wise under alpha64.DENSE_E2E (derived by (a)'s rule on THESE cases: As / Bs are other fields than A / B), the mask
    volume differing from the yardstick's only where |dilated alpha - thres| < alpha64.MASK_DELTA, such voxels at most 0.1 %, new_aabb equal
    unless such a voxel sets an extent.

Figures: bound [float32 evaluation of the yardstick, CPU] / device (abs ; rel as alpha64.floors gives them):
  (a) per time case, worst over the eleven sizes; x6 and fp32 MFMA give the same figures to the printed digits except where two are shown
      case        field A: bound [float32] / device                          field B: bound [float32] / device
      key         1.6e-7 [4.1e-8] / 3.9e-8 ; 5e-6 [1.4e-6] / 1.5e-6          1.6e-7 [3.4e-8] / 3.8e-8 ; 2e-6 [5.1e-7] / 4.3e-7
      onestep     1.6e-7 [5.1e-8] / 4.8e-8 ; 6e-6 [1.9e-6] / 2.5e-6          1.6e-7 [3.5e-8] / 3.8e-8 ; 3e-6 [7.1e-7] / 6.4e-7
      nearkey     1.6e-7 [4.7e-8] / 4.7e-8 ; 7e-6 [2.2e-6] / 2.1e-6          1.6e-7 [3.8e-8] / 3.7e-8 ; 3e-6 [9.8e-7] / 9.9e-7
      late        1.6e-7 [3.7e-8] / 3.9e-8 ; 7e-6 [2.1e-6] / 2.0e-6, 1.9e-6  1.6e-7 [3.3e-8] / 3.7e-8 ; 2e-6 [5.8e-7] / 5.8e-7
      transfer    1.6e-7 [3.3e-8] / 3.7e-8 ; 8e-6 [2.6e-6] / 2.6e-6          1.6e-7 [3.4e-8] / 3.6e-8 ; 3e-6 [8.1e-7] / 5.9e-7
      nearkey BEFORE the fix in csrc/abi.hip (the call skipped the step of a time that is only isclose to its keyframe): field A, N = 129, rel
      1.2e-5 over the bound of 7e-6 (excess 3.8e-7 on alpha 0.10); the yardstick moves 83 of 129 / 19 691 of 32 769 points by up to 1.0e-6 there
      (field B: 14 442 of 32 769 by up to 1.9e-7, inside its bound).  The undersized workspace was also accepted at a keyframe time and with the
      fp32 kernels (the 2 N floats of per-point times were only asked for on the x6 path, after the first kernel had been launched): the call now
      refuses anything under the published size before it launches.
  (b) valid counts equal in all 40 renders; 0 samples on a voxel boundary, 0 floors that differ between the two index formulas, 0 appearance-mask
      flips; no map element leaves FP32_FLOOR (largest excess over the bound -1.9e-6 on acc); the inverted decision moves a map by 1.3e-4 - 1.4e-4
      over its bound on As, block and stale in every case, on Bs by 1.2e-5 at the keyframe with R = 1 and 257 (blind in its other eight cases).
  (c) case                 bound (atol ; rtol) [float32]            device              mask voxels: differ / near      box
      As 7x5x9             2.8e-7 [3.1e-8] ; 6e-6 [1.9e-6]          3.4e-8 ; 1.9e-6     0 / 0 of 315                    equal
      As 7x5x9 transfer    2.8e-7 [3.1e-8] ; 1e-6 [3.2e-7]          3.7e-8 ; 1.8e-7
      As 33x31x29          2.8e-7 [7.9e-8] ; 2.3e-5 [7.4e-6]        8.9e-8 ; 6.9e-6     0 / 0 of 29 667                 equal
      Bs 7x5x9             2.8e-7 [9.2e-8] ; 1.2e-7 [0]             9.2e-8 ; 0          0 / 0 of 315 (all set)          equal
      Bs 7x5x9 transfer    2.8e-7 [3.2e-8] ; 2.5e-5 [8.0e-6]        3.7e-8 ; 6.9e-6
      Bs 33x31x29          2.8e-7 [8.0e-8] ; 2.9e-5 [9.6e-6]        1.2e-7 ; 8.6e-6     0 / 8 of 29 667 (0.03 %)        equal (near voxels touch the extent)
      On Bs the frame times 27/60 and 39/60 are isclose to a keyframe but not equal to it (2 of 60; every in-gate voxel takes a step of 3e-8).
The file takes about 20 s on an MI355X; no test over 2 s."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import alpha64 as a64
import render64 as r64
from conftest import GOLD
from helpers import FP32_FLOOR, field_state, load_meta, make_model
from test_gpu_render64 import MAP_RTOL

pytestmark = pytest.mark.gpu
KINDS = ["A", "B"]
SENTINEL = -7.0
TAIL = 4096
MASK_GRID = {"As": (20, 18, 16), "Bs": (33, 31, 29), "stale": (10, 9, 8)}
VOLUMES = ["As", "Bs", "block", "stale"]
RAY_COUNTS = (1, 3, 4, 5, 257)
RENDER_TIMES = (19.0 / 60.0, 0.25)
BLIND = set()        # volumes where inverting the last culling decision stays under the map bounds in every case


@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(GOLD, "r2.npz"))


@pytest.fixture(scope="module")
def plain():
    """fields A and B: the device module and the yardstick's Field of the same parameters"""
    out = {}
    for kind in KINDS:
        model, meta = make_model(kind)
        model.eval()
        out[kind] = (model, meta, r64.Field(*field_state(model)))
    return out


def _tight(g2, kind):
    """field A / B with the tight-blob parameters of r2.npz"""
    model, meta = make_model(kind)
    own = model.state_dict()
    pre = f"{kind}s:sd:"
    n = 0
    for k in g2.files:
        if k.startswith(pre) and k[len(pre):] in own:
            own[k[len(pre):]].copy_(torch.from_numpy(np.ascontiguousarray(g2[k])).cuda())
            n += 1
    assert n >= 40
    model.nvfi._fix_layout()
    model.eval()
    return model, meta


def _published(f, N):
    from nvfi_amd import _lib
    nb = C.c_int64(0)
    _lib.check(_lib.lib().nvfi_alpha_workspace_bytes(C.byref(f._desc()), C.c_int64(N), C.byref(nb)))
    return int(nb.value)


def _call(f, xyz, t, transfer, acc, out, ws, nbytes):
    from nvfi_amd import _lib
    desc = f._desc()
    rc = _lib.lib().nvfi_compute_alpha(C.byref(desc), C.c_int64(xyz.shape[0]), _lib.ptr(xyz), C.c_float(float(np.float32(t))), C.c_int(int(transfer)),
                                       C.c_float(f._step_host), C.c_int(acc), _lib.ptr(out), _lib.ptr(ws), C.c_int64(nbytes),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _excess(got, ref, rtol, atol):
    return float((np.abs(got.astype(np.float64) - ref) - rtol * np.abs(ref) - atol).max()) if len(ref) else -atol


@pytest.mark.parametrize("N", a64.SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_compute_alpha_elementwise(plain, kind, N):
    model, _, fld = plain[kind]
    f = model.nvfi
    x = a64.case_points(fld, N)
    xyz = torch.from_numpy(x).cuda().contiguous()
    nb = _published(f, N)
    bad = []
    keep_mode = f.vel_fp16
    try:
        for label, t, transfer, nsteps, every in a64.alpha_cases(fld):
            if N > a64.MULTI_STEP_MAX_N and not every:
                continue
            ref = a64.compute_alpha64(fld, x, t, transfer, f._step_host, device="cuda")
            assert len(ref["steps"]) == nsteps and ref["shortcut"] == (label == "nearkey"), (label, len(ref["steps"]), nsteps)
            edge = ref["edge"]
            assert edge.sum() <= int(0.005 * N), (label, "points near a gate face", int(edge.sum()))
            rtol, atol = a64.ALPHA_RTOL[kind][label], a64.ALPHA_ATOL
            if label == "nearkey":
                moved = np.abs(ref["xk"] - a64.normalize32(fld, x).numpy()).max(1)
                print(f"[alpha64] {kind}:{label}:N{N}: keyframe shortcut: the yardstick moves {int((moved > 0).sum())} of {N} points, by at most {moved.max():.1e}")
            for mode in ("x6", "fp32"):
                f.vel_fp16 = "fp32" if mode == "fp32" else keep_mode
                assert bool(f._desc().vel_fp16 & 8) == (mode == "fp32")
                # ---- the plain store, exactly the published size, the tail behind it
                ws = torch.full((nb + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
                out0 = torch.full((N,), SENTINEL, device="cuda")
                assert _call(f, xyz, t, transfer, 0, out0, ws, nb) == 0
                assert bool((ws[nb:] == 0xA5).all()), (label, mode, "the call wrote behind the size it publishes")
                got0 = out0.cpu().numpy()
                assert np.isfinite(got0).all() and (got0 >= 0).all() and (got0 <= 1).all(), (label, mode, "a sentinel or a value outside [0, 1] is left")
                # ---- the running maximum over values below, at and above the result
                off = np.array([-0.05, 0.0, 0.05], np.float32)[np.arange(N) % 3]
                pre = (got0 + off).astype(np.float32)
                out1 = torch.from_numpy(pre).cuda()
                assert _call(f, xyz, t, transfer, 1, out1, ws, nb) == 0
                assert bool((ws[nb:] == 0xA5).all()), (label, mode, "the call wrote behind the size it publishes")
                got1 = out1.cpu().numpy()
                assert np.array_equal(got1, np.maximum(pre, got0)), (label, mode, "accumulate_max is not max(prefill, alpha)")
                # ---- 256 bytes under the published size: refused before anything is launched
                if label in ("key", "onestep"):
                    ws2 = torch.full((nb + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
                    out2 = torch.full((N,), SENTINEL, device="cuda")
                    assert _call(f, xyz, t, transfer, 0, out2, ws2, nb - 256) == 4, (label, mode, "an undersized workspace is not refused")
                    assert bool((out2 == SENTINEL).all()) and bool((ws2 == 0x5A).all()), (label, mode, "a refused call wrote something")
                # ---- against the yardstick
                k = ~edge
                da, dr = a64.floors(got0[k], ref["alpha"][k])
                e0 = _excess(got0[k], ref["alpha"][k], rtol, atol)
                e1 = _excess(got1[k], np.maximum(pre.astype(np.float64), ref["alpha"])[k], rtol, atol)
                print(f"[alpha64] {kind}:{label}:N{N}:{mode}: {nsteps} steps, device abs {da:.2e} rel {dr:.2e} (bounds {atol:g} / {rtol:g}; error / float32 "
                      f"floor {da / (atol / 3):.2f} / {dr / (rtol / 3):.2f}), excess plain {e0:.1e} max {e1:.1e}, alpha max {ref['alpha'].max():.3f}, "
                      f"{int((ref['alpha'] > 1e-4).sum())} above 1e-4, {ref['n_rejected']} rejected steps", flush=True)
                if edge.any():
                    print(f"[alpha64] {kind}:{label}:N{N}:{mode}: near-face points {np.nonzero(edge)[0].tolist()}: device {got0[edge]}, yardstick {ref['alpha'][edge]}")
                if e0 > 0 or e1 > 0:
                    bad.append((label, mode, e0, e1, da, dr))
    finally:
        f.vel_fp16 = keep_mode
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (b) culling
def _volume_case(name, g2, plain):
    """(model, meta, kind, Field, volume (D, H, W) float32) with the volume attached to the device field"""
    from nvfi_amd.models import AlphaGridMask
    if name == "block":
        model, meta, fld = plain["A"]
        kind, vol = "A", a64.block_volume()
    else:
        kind = "B" if name == "Bs" else "A"
        model, meta = _tight(g2, kind)
        f = model.nvfi
        fld = r64.Field(*field_state(model))
        d = a64.dense_alpha64(fld, MASK_GRID[name], device="cuda")
        m = a64.update_alpha_mask64(d["alpha"], d["xyz"], float(meta["alphaMask_thres"]))
        vol = m["volume"]
        if name == "stale":
            old = f.aabb.detach().cpu().numpy().copy()
            f.alphaMask = AlphaGridMask("cuda", f.aabb, torch.from_numpy(vol).cuda())
            f.shrink(torch.from_numpy(m["new_aabb"]).cuda())
            fld = r64.Field(*field_state(model))
            assert not np.array_equal(old, fld.aabb.numpy()) and f.gridSize.tolist() != list(MASK_GRID[name]), "the box shrank, the mask did not follow"
    model.nvfi.alphaMask = AlphaGridMask("cuda", model.nvfi.aabb, torch.from_numpy(vol).cuda())
    return model, meta, kind, fld, vol


@pytest.mark.parametrize("name", VOLUMES)
def test_alpha_mask_culling(g2, gold, plain, name):
    from nvfi_amd.models import Renderer, Ray
    model, meta, kind, fld, vol = _volume_case(name, g2, plain)
    f = model.nvfi
    try:
        assert len({*vol.shape}) == 3 or name != "block"
        o = np.concatenate([gold[f"{kind}:rays_o"], gold[f"{kind}:rays_o"][:1]])
        d = np.concatenate([gold[f"{kind}:rays_d"], gold[f"{kind}:rays_d"][:1]])
        wb = bool(meta["white_background"])
        ren = Renderer(model, 0, 0, 2048)
        dims = vol.shape[::-1]
        bad, seen = [], []
        for t in RENDER_TIMES:
            for R in RAY_COUNTS:
                oc, dc = torch.from_numpy(o[:R]).cuda(), torch.from_numpy(d[:R]).cuda()
                out = ren.render(t, Ray(oc, dc, 0, 1), white_background=wb, mode="test")
                cnt = f.last_counters.cpu().numpy()
                got = dict(zip(("rgb", "depth", "acc", "weight"), (v.detach().cpu().numpy() for v in out[:4])))
                mask = got["weight"] > np.float32(fld.thres)
                kw = dict(loss=None, grads=False, alpha_volume=vol, device="cuda", app_mask=mask)
                ref = r64.render64(fld, o[:R], d[:R], t, None, wb, **kw)
                nbox, ncull = int(ref["in_box"].sum()), int(ref["culled"].sum())
                near_rays = int(ref["alpha_near"].any(1).sum())
                xn = r64.sample_rays(fld, o[:R], d[:R], None)["xn"].numpy()[ref["in_box"]]
                nfloor = int((np.floor(a64.voxel_coord(xn, dims)) != np.floor(a64.voxel_coord_device(xn, dims))).any(1).sum())
                excess = {m: float((np.abs(got[m].astype(np.float64) - ref[m]) - MAP_RTOL * np.abs(ref[m]) - FP32_FLOOR[m]).max()) for m in got}
                # sensitivity: the last in-box sample of the last ray decided the other way
                js = np.nonzero(ref["in_box"][R - 1])[0]
                moved = None
                if len(js):
                    kw1 = dict(kw, rays=[R - 1])
                    a = r64.render64(fld, o[:R], d[:R], t, None, wb, **kw1)
                    b = r64.render64(fld, o[:R], d[:R], t, None, wb, cull_flip=[(R - 1, int(js[-1]))], **kw1)
                    moved = max(float((np.abs(b[m] - a[m]) - MAP_RTOL * np.abs(a[m]) - FP32_FLOOR[m]).max()) for m in got)
                    seen.append(moved > 0)
                print(f"[alpha64] {name}:t{t:.3f}:R{R}: in box {nbox}, culled {ncull} ({ncull / max(nbox, 1):.1%}), valid: device {int(cnt[0])} yardstick "
                      f"{int(ref['valid'].sum())}; rays with a sample on a voxel boundary {near_rays}; floors that differ between the two index formulas "
                      f"{nfloor}; appearance-mask flips {len(ref['flips'])}; excess over the map bounds {({m: f'{v:.1e}' for m, v in excess.items()})}; "
                      f"the last culling decision inverted moves a map by {'-' if moved is None else f'{moved:.1e}'} over its bound", flush=True)
                if R == 257:
                    assert 0.2 <= ncull / nbox <= 0.8, (name, "the volume does not cull between 20 % and 80 %", ncull, nbox)
                assert near_rays <= int(0.005 * R), (name, R, near_rays)
                assert nfloor == 0, (name, "the two index formulas floor differently: a finding", nfloor)
                if near_rays == 0 and int(cnt[0]) != int(ref["valid"].sum()):
                    bad.append((t, R, "valid count", int(cnt[0]), int(ref["valid"].sum())))
                if len(ref["flips"]) and float(ref["flip_dist"].max()) > 2e-6:
                    bad.append((t, R, "an appearance-mask flip away from the threshold", float(ref["flip_dist"].max())))
                for m, v in excess.items():
                    if v > 0:
                        bad.append((t, R, m, v))
        assert not bad, bad
        if name in BLIND:
            assert not any(seen), (name, "is listed as blind but is not")
        else:
            assert any(seen), (name, "no case sees the last culling decision")
    finally:
        f.alphaMask = None


# ---------------------------------------------------------------------------------------------------------------- (c) end to end
def mask_flips_only_near(vol, alpha64_volume, xyz, thres, label):
    """the device's mask volume (D, H, W) against the yardstick's from the float64 dense alpha: flips only where the yardstick's margin is under
    MASK_DELTA, such voxels at most 0.1 %; returns (yardstick mask dict, near voxels)"""
    m = a64.update_alpha_mask64(alpha64_volume, xyz, thres)
    near = m["margin"] < a64.MASK_DELTA
    diff = np.asarray(vol).reshape(m["volume"].shape) != m["volume"]
    print(f"[alpha64] {label}: mask voxels that differ {int(diff.sum())}, within {a64.MASK_DELTA:g} of the threshold {int(near.sum())} of {near.size}"
          + (f", margins of the differing ones {m['margin'][diff]}" if diff.any() else ""))
    assert not (diff & ~near).any(), (label, "a mask voxel flipped away from the threshold", m["margin"][diff & ~near])
    assert near.sum() <= 1e-3 * near.size, (label, int(near.sum()))
    return m, near


@pytest.mark.parametrize("grid", [(7, 5, 9), (33, 31, 29)])
@pytest.mark.parametrize("kind", KINDS)
def test_dense_alpha_and_mask_end_to_end(g2, kind, grid):
    model, meta = _tight(g2, kind)
    f = model.nvfi
    fld = r64.Field(*field_state(model))
    thres = float(meta["alphaMask_thres"])
    try:
        for transfer in ([False, True] if grid[0] == 7 else [False]):
            rtol, atol = a64.DENSE_E2E[(kind, grid[0], transfer)]
            alpha, _ = f.getDenseAlpha(list(grid), transfer=transfer)
            got = alpha.cpu().numpy()
            d = a64.dense_alpha64(fld, grid, transfer, device="cuda")
            k = ~d["edge"]
            da, dr = a64.floors(got[k], d["alpha"][k])
            e = _excess(got[k], d["alpha"][k], rtol, atol)
            print(f"[alpha64] {kind}s:{grid}:{'transfer' if transfer else 'plain'}: device abs {da:.2e} rel {dr:.2e} (bounds {atol:g} / {rtol:g}), excess {e:.1e}; "
                  f"{int(d['edge'].sum())} voxels near a gate face; {len(d['shortcut_times'])} of 60 frame times are isclose to a keyframe but not equal to it", flush=True)
            assert got.shape == tuple(grid) and e <= 0, (kind, grid, transfer, da, dr)
            if transfer:
                continue
            new_aabb = f.updateAlphaMask(list(grid)).cpu().numpy()
            vol = f.alphaMask.alpha_volume.cpu().numpy()
            assert vol.shape[-3:] == tuple(grid)[::-1]
            m, near = mask_flips_only_near(vol, d["alpha"], d["xyz"], thres, f"{kind}s:{grid}")
            sets_extent = a64.aabb_near(m["volume"], near, d["xyz"])
            print(f"[alpha64] {kind}s:{grid}: {m['volume'].mean():.3f} of the volume set; a near voxel sets an extent of the box: {sets_extent}")
            assert np.array_equal(new_aabb, m["new_aabb"]) or sets_extent, (new_aabb, m["new_aabb"])
    finally:
        f.alphaMask = None
