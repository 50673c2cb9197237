"""Float64 restatement of the occupancy path of the reference's TensorVMKeyframeTimeKplane: compute_alpha (models/tensorf_keyframe.py:508-537),
getDenseAlpha (:461-499), updateAlphaMask (:379-405) and AlphaGridMask.sample_alpha (models/tensorf_model_utils.py:433-439) - the yardstick of
tests/test_alpha64_golden.py (against the reference's goldens) and of tests/test_gpu_alpha64.py (against include/nvfi_hip.h: nvfi_compute_alpha,
field.getDenseAlpha / updateAlphaMask and render_rays.hip: alpha_lookup).  Built from render64.time_plan / _planes / _vel, advect64.rk2_back (the
one RK2 loop with its gate, rejection and near-face bookkeeping) and flow64._near_face.  Written out from the mathematics:

  compute_alpha: x = normalize_coord(world point); base = round(clamp(t / dt_k, 0, K - 1)) dt_k (0 with transfer); x_k = integrate_pos(x, t, base);
      alpha = 1 - exp(-softplus(density feature(x_k, normalised base) + density_shift) * length).
  getDenseAlpha: the grid aabb0 (1 - s) + aabb1 s, s = linspace(0, 1, g) per axis, the maximum of compute_alpha over the 60 times i / 60.
  updateAlphaMask: clamp to [0, 1], 3^3 max-pool (stride 1, padding 1), >= alphaMask_thres -> 1 else 0, stored (D, H, W) = (z, y, x); the returned
      box is the per-axis min / max of the grid points of the voxels that are set.
  sample_alpha: F.grid_sample of that volume, trilinear, align_corners=True, zeros padding, at the FIELD's normalised coordinates.

As in render64, what the reference computes in fp32 before it touches the field stays fp32-rounded and is then promoted (the grid, the normalised
points, t, the base time, the step schedule, length), every discrete decision is taken on fp32-rounded values, the rest runs in `dtype`; dtype =
float32 is "a plain fp32 implementation" of the same statement, whose distance from the float64 run is the floor the bounds are derived from.

Three places where the device did or might not do literally what is written above - each restated HERE the reference's way, so that the comparison measures it:
  * Keyframe shortcut.  The reference's compute_alpha has no isclose(t, base) shortcut: integrate_pos steps while t - base != 0.  nvfi_compute_alpha
    took no step when is_close(t, base) (the render's rk_schedule) until this yardstick measured it: at t = 0.25 (1 + 4e-6) on field A the tiny step
    (|dt| <= 1e-8 + 1e-5 |base|) moves 83 of 129 points by up to 9.4e-7 and alpha by 1.2e-5 relative, over the case's derived 7e-6.  The call now
    follows the reference (csrc/abi.hip); `shortcut` in compute_alpha64's result marks the calls where the two used to part.
  * Index arithmetic.  ATen's grid_sampler_unnormalize forms ((x + 1) / 2) (W - 1); alpha_lookup forms (x + 1) ((W - 1) / 2).  The halving is exact
    in both, so both are ONE rounding of the same real product and agree bit for bit (voxel_coord / voxel_coord_device: counted by the tests, 0 of
    every sample they see).  What does differ by an ulp is the normalised coordinate itself where the compiler contracts (p - aabb0) inv - 1 into a
    fused multiply-add; sample_alpha64 reports how close a coordinate is to an integer for that reason.
  * Mask coordinates.  sample_alpha has its own normalize_coord commented out and reads the volume with the field's normalised coordinates: after
    shrink() a mask built in the old box is read in NEW-box coordinates, by the reference and by the device alike.  render64(alpha_volume=...)
    restates exactly that: it passes its own xn."""
import numpy as np
import torch
import torch.nn.functional as F

import advect64
import render64 as r64

NEAR_ULP = 4      # a voxel coordinate within this many fp32 ulp (of W - 1, the coordinate's scale) of an integer may floor the other way


def field_from_npz(z, prefix, meta):
    """render64.Field of the tight-blob parameters `<prefix>sd:nvfi.*` of tests/golden/r2.npz under the configuration of field A / B"""
    sd = {k[len(prefix) + 3:]: z[k] for k in z.files if k.startswith(prefix + "sd:")}
    return r64.Field(sd, dict(meta, aabb=sd["nvfi.aabb"]))


def normalize32(field, xyz_world):
    """normalize_coord in fp32: (p - aabb0) * (2 / size) - 1, each operation rounded"""
    p = torch.as_tensor(np.asarray(xyz_world, np.float32)).reshape(-1, 3)
    a0, a1 = field.aabb[0], field.aabb[1]
    return (p - a0) * (2.0 / (a1 - a0)) - 1


def compute_alpha64(field, xyz_world, t, transfer=False, length=None, dtype=torch.float64, device="cpu"):
    """dict: alpha (N,) numpy in `dtype`, xk (the warped points), edge (bool per point: a gate or rejection decision within 4 fp32 ulp of a face),
    steps (the schedule actually taken), shortcut (the device takes none of them: isclose(t, base) but t != base), base, n_rejected"""
    xn = normalize32(field, xyz_world)
    plan = r64.time_plan(field, t, transfer)
    steps = advect64.schedule(field, t, plan["base"])          # integrate_pos' own loop: no isclose shortcut
    assert plan["key"] or steps == plan["steps"], "time_plan and the schedule disagree"
    length = field.step if length is None else float(np.float32(length))
    with torch.no_grad():
        P = {k: v.to(device=device, dtype=dtype) for k, v in field.p32.items() if k in r64.VEL_NAMES or k.startswith("density")}
        xk, info = advect64.rk2_back(P, field, xn.to(device=device, dtype=dtype), steps, dtype)
        x4 = torch.cat([xk, torch.full_like(xk[:, :1], plan["tn_base"])], 1)
        sigma = F.softplus(r64._planes(P, "density", x4).sum(0) + field.shift)
        alpha = 1.0 - torch.exp(-sigma * length)
    return dict(alpha=alpha.cpu().numpy(), xk=xk.cpu().numpy(), edge=info["edge"], steps=steps, shortcut=bool(plan["key"] and steps),
                base=plan["base"], n_rejected=info["n_rejected"])


# ---------------------------------------------------------------------------------------------------------------- the volume lookup
def voxel_coord(xn32, dims):
    """(n, 3) fp32 numpy: ATen's grid_sampler_unnormalize, align_corners=True: ((x + 1) / 2) * (size - 1); dims = (W, H, D)"""
    x = np.asarray(xn32, np.float32)
    return ((x + np.float32(1)) / np.float32(2)) * (np.asarray(dims, np.float32) - np.float32(1))


def voxel_coord_device(xn32, dims):
    """the same in alpha_lookup's order of operations: (x + 1) * ((size - 1) / 2)"""
    x = np.asarray(xn32, np.float32)
    return (x + np.float32(1)) * ((np.asarray(dims, np.float32) - np.float32(1)) / np.float32(2))


def _trilinear(vol, fl, fr):
    """sum over the eight corners of vol (D, H, W) at integer floors fl (n, 3) = (x, y, z) with fractions fr (n, 3), zeros outside"""
    D, H, W = vol.shape
    out = torch.zeros(fl.shape[0], dtype=vol.dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = fl[:, 0] + dx, fl[:, 1] + dy, fl[:, 2] + dz
                ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & (zi >= 0) & (zi < D)
                w = (fr[:, 0] if dx else 1 - fr[:, 0]) * (fr[:, 1] if dy else 1 - fr[:, 1]) * (fr[:, 2] if dz else 1 - fr[:, 2])
                v = vol[zi.clamp(0, D - 1), yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
                out = out + torch.where(ok, v * w, torch.zeros_like(w))
    return out


def sample_alpha64(volume, xn, dtype=torch.float64):
    """the lookup of a (D, H, W) volume at the fp32 normalised points xn (n, 3) -> alpha (n,) numpy in `dtype`, ulps (n, 3): the distance of each
    voxel coordinate from the nearest integer in fp32 ulp of its scale (size - 1), near (n,) bool: some coordinate lies within NEAR_ULP of an
    integer k AND the decision alpha > 0 changes when that coordinate is placed just below k (corners k - 1, k), on k (corner k alone) or just
    above it (corners k, k + 1).  The volume is non-negative, so only which corners carry weight matters for the decision."""
    vol = torch.as_tensor(np.asarray(volume)).reshape(np.asarray(volume).shape[-3:])
    D, H, W = vol.shape
    dims = (W, H, D)
    x32 = (xn.detach().cpu().numpy() if torch.is_tensor(xn) else np.asarray(xn)).astype(np.float32).reshape(-1, 3)
    ix = voxel_coord(x32, dims)
    fl32 = np.floor(ix)
    fl = torch.from_numpy(np.clip(fl32, -4, np.asarray(dims, np.float32) + 2).astype(np.int64))       # (far outside: every corner is padding)
    fr = torch.from_numpy((ix.astype(np.float64) - fl32.astype(np.float64))).to(dtype)
    alpha = _trilinear(vol.to(dtype), fl, fr)
    k = np.rint(ix)
    ulps = np.abs(ix.astype(np.float64) - k) / np.spacing(np.asarray(dims, np.float32) - np.float32(1)).astype(np.float64)
    near_c = ulps <= NEAR_ULP
    near = np.zeros(len(x32), bool)
    rows = np.nonzero(near_c.any(1))[0]
    if rows.size:
        own = (alpha[rows] > 0).numpy()
        kk = torch.from_numpy(np.clip(k[rows], -4, np.asarray(dims, np.float32) + 2).astype(np.int64))
        nc = torch.from_numpy(near_c[rows])
        half = torch.full((len(rows),), 0.5, dtype=dtype)
        zero = torch.zeros(len(rows), dtype=dtype)
        alts = [(kk - 1, half), (kk, zero), (kk, half)]
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    f2, r2 = fl[rows].clone(), fr[rows].clone()
                    for ax, ch in enumerate((a, b, c)):
                        f2[:, ax] = torch.where(nc[:, ax], alts[ch][0][:, ax], f2[:, ax])
                        r2[:, ax] = torch.where(nc[:, ax], alts[ch][1], r2[:, ax])
                    near[rows] |= (_trilinear(vol.to(dtype), f2, r2) > 0).numpy() != own
    return alpha.numpy(), ulps, near


# ---------------------------------------------------------------------------------------------------------------- grid maintenance
def dense_grid(field, grid):
    """(g0, g1, g2, 3) fp32: aabb0 (1 - s) + aabb1 s with s the meshgrid of linspace(0, 1, g) ('ij')"""
    s = torch.stack(torch.meshgrid(*[torch.linspace(0, 1, int(g)) for g in grid], indexing="ij"), -1)
    return field.aabb[0] * (1 - s) + field.aabb[1] * s


FRAME_TIMES = [float(np.float32(v)) for v in np.linspace(0, 59, 60) / 60]      # (the reference multiplies an fp32 tensor of ones by each)


def dense_alpha64(field, grid, transfer=False, dtype=torch.float64, device="cpu", times=None):
    """dict: alpha (g0, g1, g2) numpy in `dtype`: the maximum over the 60 frame times; xyz (the grid, fp32 torch); edge (bool per voxel: near a face
    at some time); shortcut_times (the frame times at which the device's keyframe shortcut applies and the reference steps)"""
    xyz = dense_grid(field, grid)
    flat = xyz.reshape(-1, 3)
    alpha, edge, short = None, np.zeros(flat.shape[0], bool), []
    for t in (FRAME_TIMES if times is None else times):
        r = compute_alpha64(field, flat, t, transfer, field.step, dtype, device)
        alpha = r["alpha"] if alpha is None else np.maximum(alpha, r["alpha"])
        edge |= r["edge"]
        if r["shortcut"]:
            short.append(t)
    shape = tuple(int(g) for g in grid)
    return dict(alpha=alpha.reshape(shape), xyz=xyz, edge=edge.reshape(shape), shortcut_times=short)


def update_alpha_mask64(alpha, xyz, thres):
    """dict: volume (D, H, W) float32 of 0 / 1, new_aabb (2, 3) float32, margin (D, H, W) float64 = |dilated alpha - thres|, dilated.  alpha in any
    float dtype; the threshold is the fp32 rounding of alphaMask_thres (an fp32 tensor against a Python scalar compares in fp32)"""
    a = torch.as_tensor(np.asarray(alpha))
    th = float(np.float32(thres))
    g = a.shape
    dil = F.max_pool3d(a.clamp(0, 1).transpose(0, 2).contiguous()[None, None], kernel_size=3, padding=1, stride=1).view(g[2], g[1], g[0])
    vol = (dil >= th).to(torch.float32)
    pts = xyz.transpose(0, 2)[vol > 0.5]
    new_aabb = torch.stack((pts.amin(0), pts.amax(0))) if len(pts) else torch.full((2, 3), float("nan"))
    return dict(volume=vol.numpy(), new_aabb=new_aabb.numpy(), margin=np.abs(dil.to(torch.float64).numpy() - th), dilated=dil.numpy())


def aabb_near(mask, near, xyz):
    """True if un-setting or setting any `near` voxel of the mask (D, H, W) could move the box of update_alpha_mask64: some near voxel lies on or
    outside the per-axis extent of the voxels that are set and not near"""
    sure = (np.asarray(mask) > 0.5) & ~near
    if not near.any():
        return False
    if not sure.any():
        return True
    idx_s, idx_n = np.argwhere(sure), np.argwhere(near)
    return bool(((idx_n <= idx_s.min(0)) | (idx_n >= idx_s.max(0))).any())


# ---------------------------------------------------------------------------------------------------------------- inputs of the test cases
def block_volume(dims=(37, 50, 41), block=(6, 7, 5)):
    """a synthetic (D, H, W) occupancy volume of 0 / 1 in a 3-D checker of blocks; dims = (W, H, D), all different, so that a transposed or
    mis-sized read cannot reproduce it"""
    W, H, D = dims
    k, j, i = np.meshgrid(np.arange(D) // block[2], np.arange(H) // block[1], np.arange(W) // block[0], indexing="ij")
    return ((i + j + k) % 2).astype(np.float32)


def case_points(field, N):
    """world points of a compute_alpha case: uniform over 1.15 x the box (some normalise beyond +-1: the gate holds them still and the planes
    are read through their zero padding); from N = 31 on the first nine are the centre of a face, two corners, an edge and points of the faces"""
    rng = np.random.default_rng(211 + N)
    a0, a1 = field.aabb[0].numpy().astype(np.float64), field.aabb[1].numpy().astype(np.float64)
    c, h = (a0 + a1) / 2, (a1 - a0) / 2
    x = (c + (rng.random((N, 3)) * 2 - 1) * 1.15 * h).astype(np.float32)
    if N >= 31:
        a0, a1 = field.aabb[0].numpy(), field.aabb[1].numpy()
        c32 = c.astype(np.float32)
        x[0] = a0
        x[1] = a1
        x[2] = (a0[0], c32[1], c32[2])
        x[3] = (c32[0], a1[1], c32[2])
        x[4] = (a1[0], a1[1], c32[2])
        x[5] = (x[5][0], x[5][1], a0[2])
        x[6] = (x[6][0], a0[1], x[6][2])
        x[7] = (a1[0], x[7][1], x[7][2])
        x[8] = (a0[0], a1[1], a0[2])
    return x


def near_key_time(field, k=1):
    """a time that is isclose to keyframe k but not equal to it: base (1 + 4e-6) in fp32"""
    base = np.float32(k * (field.tmax / (field.K - 1)))
    return float(np.float32(base * np.float32(1 + 4e-6)))


def floors(a32, a64):
    """(abs, rel) of a float32 evaluation (or the device) against the float64 one: abs = max |err| over the elements with |ref| <= 1e-2, where the
    cancellation of 1 - exp(-x) decides (half an ulp of 1.0 whatever x); rel = max (|err| - abs) / |ref| over all elements, what is left for the
    relative error of sigma.  A bound rtol |ref| + atol with atol >= abs and rtol >= rel holds every element."""
    a32, a64 = np.asarray(a32, np.float64).ravel(), np.asarray(a64, np.float64).ravel()
    err = np.abs(a32 - a64)
    small = np.abs(a64) <= 1e-2
    A = float(err[small].max()) if small.any() else 0.0
    big = np.abs(a64) > 0
    r = float(np.maximum(err[big] - A, 0).__truediv__(np.abs(a64[big])).max()) if big.any() else 0.0
    return A, r


SIZES = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 32769)
MULTI_STEP_MAX_N = 257


def alpha_cases(field):
    """[(label, t, transfer, RK2 steps of the yardstick, every size?)] of the element-wise compute_alpha cases.  The step counts follow from
    dt_max = tmax / (2 (K - 1)): field A (K = 4, tmax = 0.75) 0.125, field B (K = 16) 0.025; `nearkey` is isclose to keyframe 1 but not equal to
    it: the yardstick takes the reference's one tiny step, the device none."""
    dtm = 0.5 * field.tmax / (field.K - 1)
    return [("key", 0.25, False, 0, True),
            ("onestep", 19.0 / 60.0, False, 1, True),
            ("nearkey", near_key_time(field), False, 1, True),
            ("late", 0.93, False, int(np.ceil((0.93 - 0.75) / dtm)), False),
            ("transfer", 59.0 / 60.0, True, int(np.ceil((59.0 / 60.0) / dtm)), False)]


# The bounds the device is held to per element-wise case, |got - ref| <= rtol |ref| + atol: 3 x the plain-fp32 floor of the statement above, floors()
# of compute_alpha64(float32) against compute_alpha64(float64), worst over SIZES, measured on the CPU (torch 2.10) and rounded up;
# tests/test_alpha64_golden.py measures the floors again and fails when 3 x one of them exceeds its entry here.  Measured (abs, rel):
#   A: key 4.1e-8, 1.4e-6   onestep 5.1e-8, 1.9e-6   nearkey 4.7e-8, 2.2e-6   late 3.7e-8, 2.1e-6   transfer 3.3e-8, 2.6e-6
#   B: key 3.4e-8, 5.1e-7   onestep 3.5e-8, 7.1e-7   nearkey 3.8e-8, 9.8e-7   late 3.3e-8, 5.8e-7   transfer 3.4e-8, 8.1e-7
ALPHA_ATOL = 1.6e-7
ALPHA_RTOL = {"A": dict(key=5e-6, onestep=6e-6, nearkey=7e-6, late=7e-6, transfer=8e-6),
              "B": dict(key=2e-6, onestep=3e-6, nearkey=3e-6, late=2e-6, transfer=3e-6)}
# the dense volumes of the tight-blob fields (the maximum over 60 frame times): measured 4.3e-8, 3.9e-6 (As), 6.5e-8, 7.3e-6 (As transfer),
# 6.7e-8, 7.5e-6 (Bs) on the golden grids; the relative figure is the cancellation of 1 - exp(-x) just above floors()' 1e-2 split, not sigma
DENSE_ATOL = 2.1e-7
DENSE_RTOL = 2.3e-5
# a mask voxel may differ only where |dilated alpha - thres| < MASK_DELTA: 3 x the float32 floor of alpha within a decade of the threshold 1e-4
# (3.3e-8 on As, As transfer and Bs alike: half an ulp of exp(-x) next to 1.0), rounded up
MASK_DELTA = 1e-7
# getDenseAlpha end to end on the tight-blob fields, (kind, first grid extent, transfer) -> (rtol, atol), by the same rule on those cases (other
# fields than A / B, and a maximum over 60 times): measured floors (abs, rel): As 7x5x9 3.1e-8, 1.9e-6; transfer 3.1e-8, 3.2e-7; As 33x31x29 7.9e-8,
# 7.4e-6; Bs 7x5x9 9.2e-8, 0 (every alpha of that grid is large: the absolute part takes all of it); transfer 3.2e-8, 8.0e-6; Bs 33x31x29 8.0e-8,
# 9.6e-6.  One atol for all six, 3 x the worst (the rounding of exp(-x) next to 1.0 does not depend on the case); no rtol under one fp32 ulp.
DENSE_E2E_ATOL = 2.8e-7
DENSE_E2E = {("A", 7, False): (6e-6, DENSE_E2E_ATOL), ("A", 7, True): (1e-6, DENSE_E2E_ATOL), ("A", 33, False): (2.3e-5, DENSE_E2E_ATOL),
             ("B", 7, False): (1.2e-7, DENSE_E2E_ATOL), ("B", 7, True): (2.5e-5, DENSE_E2E_ATOL), ("B", 33, False): (2.9e-5, DENSE_E2E_ATOL)}
