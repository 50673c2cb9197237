"""Edge cases of the hot path on the GPU: ragged and empty inputs, rays that miss the box, a fully transparent field (the PDE
keeps no point, as at the reference's initialisation), and the largest configuration of the shipped schedule (199^3 grid with
step_ratio 0.5 -> 686 samples per ray, ~1.4 M samples per 2048-ray chunk)."""
import numpy as np
import pytest
import torch

from helpers import make_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    return make_model("A")


def _rays(n, seed=0, miss=False):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([[2.6, -2.2, 2.4]]).expand(n, 3).contiguous()
    tgt = (torch.rand(n, 3, generator=g) - 0.5) * 3.0
    if miss:
        tgt = tgt + torch.tensor([[40.0, 40.0, 0.0]])      # pointing far away from the box
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.cuda(), d.contiguous().cuda()


@pytest.mark.parametrize("n", [0, 1, 3, 63, 65, 129, 2049])
def test_ragged_ray_counts(small, n):
    """sizes that are not multiples of the wave / workgroup / chunk granularity: every prefix of a render equals the render"""
    model, meta = small
    f = model.nvfi
    f.eval()
    o, d = _rays(2049, 1)
    with torch.no_grad():
        full = f(0.41, o, d, True)
        part = f(0.41, o[:n].contiguous(), d[:n].contiguous(), True)
    assert torch.equal(part[0], full[0][:n]) and torch.equal(part[1], full[1][:n]) and torch.equal(part[3], full[3][:n])


def test_rays_that_miss_the_box(small):
    model, meta = small
    f = model.nvfi
    o, d = _rays(256, 2, miss=True)
    f.train()
    model.zero_grad(set_to_none=True)
    out = f(0.41, o, d, True)
    assert int(f.last_counters[0]) == 0 and int(f.last_counters[2]) == 0          # no valid sample, nothing masked in
    assert torch.equal(out[2], torch.zeros_like(out[2]))                           # acc = 0
    assert torch.allclose(out[0], torch.ones_like(out[0]))                         # white background
    assert torch.allclose(out[1], torch.full_like(out[1], float(meta["far"])))     # depth = far
    out[0].sum().backward()                                                        # backward with empty sample lists
    for p in model.parameters():
        assert p.grad is None or (torch.isfinite(p.grad).all() and float(p.grad.abs().max()) == 0.0)


def test_transparent_field_keeps_no_pde_point():
    """reference behaviour at initialisation (nvfi.py:66-67): get_vel_loss returns the python float 0."""
    model, meta = make_model("A")
    f = model.nvfi
    with torch.no_grad():
        for p in f.density_plane_space:
            p.zero_()                                   # sigma = softplus(-10) ~ 4.5e-5 -> alpha < 1e-4 everywhere
    g = torch.Generator(device="cuda").manual_seed(0)
    mn, mx = f.aabb
    pts = torch.rand(4096, 3, device="cuda", generator=g) * (mx - mn) + mn
    tt = torch.rand(4096, 1, device="cuda", generator=g)
    lv = model.get_vel_loss(points=pts, t=tt)
    assert isinstance(lv, float) and lv == 0.0
    assert int(f.last_pde_n_kept) == 0


def test_largest_shipped_configuration():
    """199^3 grid, step_ratio 0.5, max_n_samples 1024 -> nSamples = 686: train fwd + bwd on a full 2048-ray chunk, finite
    gradients everywhere, composite identities, and chunking invariance of the eval render.  (The values: tests/test_gpu_render64.py, case
    big686, holds a 256-ray subset of this configuration to the float64 reference.)"""
    import bench
    from nvfi_amd.models import NVFi
    cfg = bench.bat_cfg(1024, True)
    torch.manual_seed(233)
    m = NVFi(cfg, "cpu", torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]]), [199, 199, 199], [1.0, 8.0])
    f = m.nvfi
    with torch.no_grad():
        for i in range(3):
            p = f.density_plane_space[i]
            H, W = p.shape[-2:]
            yy = torch.linspace(-1, 1, H)[:, None]; xx = torch.linspace(-1, 1, W)[None, :]
            p.mul_((3.2 * torch.sqrt(torch.exp(-xx ** 2 / (2 * 0.35 ** 2)) * torch.exp(-yy ** 2 / (2 * 0.35 ** 2))))[None, None])
    m = m.cuda()
    assert f.nSamples == 686, f.nSamples
    o, d = bench.camera_bundle(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(4)
    idx = torch.randint(0, o.shape[0], (2048,), device="cuda", generator=g)
    ro, rd = o[idx].contiguous(), d[idx].contiguous()
    f.train()
    out = f(19.0 / 60.0, ro, rd, True)
    V = int(f.last_counters[0])
    assert V > 0.3 * 2048 * 686 and out[3].shape == (2048, 686)
    assert torch.allclose(out[3].sum(-1), out[2], rtol=1e-5, atol=1e-6)
    (out[0].square().mean() + 0.01 * out[1].mean()).backward()
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name
    assert float(f.density_plane_space[0].grad.abs().max()) > 0 and float(f.vel_net.weight_net[4][0].weight.grad.abs().max()) > 0
    f.eval()
    with torch.no_grad():
        full = f(0.32, ro, rd, True)
        a = f(0.32, ro[:700].contiguous(), rd[:700].contiguous(), True)
    assert torch.equal(a[0], full[0][:700])


def test_atomic_scatter_fallback_still_matches_goldens():
    """The sorted-tile scatter falls back to the atomic kernels for grids with more than 6144 tiles; that path (also selectable
    with NVFI_SCATTER_TILES=0, read once per process) must keep passing the gradient goldens."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, NVFI_SCATTER_TILES="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_render_train_grads or test_inplace_gradient_accumulation"], env=env, cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("grid", [(37, 50, 41), (7, 5, 9), (130, 97, 61)])
def test_scatter_kernels_agree(tmp_path, grid):
    """The three plane-gradient scatters - MFMA on 4x4-texel tiles (default), LDS read-add-write on 8x8 tiles (NVFI_SCATTER=lds), global
    atomics (NVFI_SCATTER_TILES=0) - sum the same fp32 products in different orders: all twelve plane gradients of a keyframe and a
    non-keyframe backward agree to summation-order noise on grids with partial edge tiles on every axis (37x50x41, 130x97x61) and on one
    with fewer texels than a tile along an axis (7x5x9)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for mode, env in (("mfma", dict(NVFI_SCATTER="mfma")), ("lds", dict(NVFI_SCATTER="lds")), ("atomic", dict(NVFI_SCATTER_TILES="0"))):
        out = str(tmp_path / f"{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "scatter_modes_worker.py"), out] + [str(g) for g in grid], env=dict(os.environ, **env),
                           cwd=os.path.join(root, "tests"), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[mode] = dict(np.load(out))
    for name, ref in got["atomic"].items():
        assert float(np.abs(ref).max()) > 0, name
        for mode in ("mfma", "lds"):
            err = float(np.linalg.norm(got[mode][name] - ref) / np.linalg.norm(ref))
            worst = float(np.abs(got[mode][name] - ref).max() / np.abs(ref).max())
            assert err < 3e-6 and worst < 1e-5, (mode, name, err, worst)


def test_fast_activation_and_trig_error_bounds():
    """engine.h replaces libm on the hot path: `fast_sigmoid` (v_exp_f32 + v_rcp_f32) and `trig_sel` (3-constant Cody-Waite reduction +
    minimax kernels).  Direct error bounds against float64 over the argument ranges the path produces: pre-activations |z| <= 40;
    encoder arguments |a| <= 40 (render PE: |coordinate| <= 1.2 times 2^5; velocity encoder: times 2^2), checked out to 400."""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(kind, x):
        xd = torch.from_numpy(x).cuda()
        y = torch.empty_like(xd)
        _lib.check(L.nvfi_debug_act(C.c_int(kind), C.c_int64(xd.numel()), _lib.ptr(xd), _lib.ptr(y), st))
        return y.cpu().numpy().astype(np.float64)

    rng = np.random.default_rng(0)
    z = np.concatenate([rng.uniform(-40, 40, 1 << 20), rng.normal(0, 2, 1 << 20), np.linspace(-100, 100, 4001)]).astype(np.float32)
    z64 = z.astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-z64))
    got = run(0, z)
    inr = np.abs(z64) <= 80.0           # beyond that exp(-z) overflows fp32 in the reference's own `1 / (1 + exp(-z))` as well: both give exactly 0
    rel = np.abs(got[inr] - s[inr]) / s[inr]
    print("fast_sigmoid max rel err (|z| <= 80)", rel.max(), "max abs err elsewhere", np.abs(got[~inr] - s[~inr]).max())
    assert rel.max() < 1e-5             # ~2e-7 + |z| 6e-8 by construction (two ~1-ulp hardware ops); far inside the 1e-4 contract
    assert np.abs(got[~inr] - s[~inr]).max() < 1e-30
    for kind, ref in ((3, z64 * s), (4, s * (1 + z64 * (1 - s))), (5, s * (1 - s) * (2 + z64 * (1 - 2 * s)))):
        got = run(kind, z)
        # fp32 evaluation of s (1 + z (1 - s)) cancels near the zero of SiLU' (z = -1.28) whatever the sigmoid: the bound is a few ulp of
        # the O(1) intermediates (absolute) + 1e-5 relative
        # (and `1 - s` carries an absolute 6e-8 for z >~ 10, which SiLU'' multiplies by |2 - z|)
        floor = 5e-7 if kind != 5 else 2e-6
        err = np.abs(got - ref) / (1e-5 * np.abs(ref) + floor)
        print("act kind", kind, "max err / (1e-5 |ref| + floor)", err.max())
        assert err.max() < 1.0, (kind, err.max())
    for lim, tol_ulp in ((40.0, 2.0), (400.0, 2.5)):
        a = np.concatenate([rng.uniform(-lim, lim, 1 << 20), np.linspace(-lim, lim, 8001)]).astype(np.float32)
        a64 = a.astype(np.float64)
        for kind, ref in ((1, np.sin(a64)), (2, np.cos(a64))):
            got = run(kind, a)
            ulp = np.abs(got - ref) / np.spacing(np.maximum(np.abs(ref), 2.0 ** -24).astype(np.float32)).astype(np.float64)
            abs_err = np.abs(got - ref)
            print(f"trig_sel kind {kind} |a|<={lim}: max abs err {abs_err.max():.3e}, max ulp {ulp.max():.2f}")
            assert abs_err.max() < 2.5e-7, (kind, lim, abs_err.max())       # absolute: what enters the MLP's first layer
            assert np.percentile(ulp, 99.9) <= tol_ulp + 1.0, (kind, lim, np.percentile(ulp, 99.9))


def test_deterministic_mode():
    """NVFI_DETERMINISTIC=1: the plane-gradient scatter accumulates fixed-point integers, so three backward passes over
    2048 rays that all cross the same texels give BIT-IDENTICAL gradients for every parameter (planes, basis, render MLP, velocity net),
    and the numbers still match the reference goldens."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "det_check.py")], env=dict(os.environ, NVFI_DETERMINISTIC="1"), cwd=root,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    bad = [k for k, v in res["bit_identical"].items() if not v]
    assert not bad, bad
    assert len(res["bit_identical"]) >= 30
    assert res["worst_relerr_vs_reference"] < 5e-4, res["worst_relerr_vs_reference"]


@pytest.mark.parametrize("env", [dict(NVFI_BWD_FORK="0"), dict(NVFI_SCATTER="lds"), dict(NVFI_RK2_FUSE="0"), dict(NVFI_PDE_FUSE="0")],
                         ids=["no_bwd_fork", "scatter_lds", "rk2_adjoint_and_wgrad_unfused", "pde_adjoint_and_wgrad_unfused"])
def test_round3_switches_keep_the_goldens(env):
    """the alternatives that are still shipped beside the defaults - the keyframe backward on one stream instead of the forked density half, the LDS
    read-add-write tile scatter instead of the MFMA one, and the unfused adjoints (k_rk2_split_bwd / k_pde_jet_bwd with k_wgrad_ring8 over the full
    adjoint stash: the A/B references of the persistent kernels) - under the gradient goldens.  (Round 6 retired the other switches of rounds 1-4
    with their kernels: the register-operand k_wgrad, the column-parallel Jacobian kernels, the one-tile-per-wave RK2 kernels with their adjoint,
    and the sweep knobs of the split kernels - INTEGRATION.md section 4 keeps the list.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), os.path.join(root, "tests", "test_cfg2.py"),
                        "-q", "-x", "-m", "gpu", "-k", "train_grads or pde_loss or mask_branch or cfg2"], env=dict(os.environ, **env), cwd=root,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("shape", [(1,), (2048, 3), (4099, 3)])
def test_fused_mse_matches_torch(shape):
    """nvfi_mse (value + gradient of F.mse_loss in one launch; bench.py's fused driver) against torch, with an upstream factor"""
    import torch
    from nvfi_amd.utils import mse_loss
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(*shape, device="cuda", generator=g, requires_grad=True)
    y = torch.rand(*shape, device="cuda", generator=g)
    x2 = x.detach().clone().requires_grad_()
    (3.0 * mse_loss(x, y)).backward()
    (3.0 * torch.nn.functional.mse_loss(x2, y)).backward()
    assert torch.allclose(mse_loss(x, y).detach(), torch.nn.functional.mse_loss(x2, y).detach(), rtol=2e-6, atol=0)
    assert torch.allclose(x.grad, x2.grad, rtol=1e-6, atol=1e-9)
    assert mse_loss(x.detach().cpu(), y.cpu()).item() == torch.nn.functional.mse_loss(x.detach().cpu(), y.cpu()).item()      # CPU tensors: torch


@pytest.mark.parametrize("P", [33, 1000, 262144 + 4133], ids=["one_tile", "fewer_tiles_than_cus", "two_chunks"])
def test_pde_gradients_add_up_over_ragged_point_sets(P):
    """The PDE term is a mean over the kept points, so n_kept * (value, gradient) of a point set equals the sum over any partition of it.  Checked for
    the shapes the persistent adjoint kernel (pde_fuse.hip) treats specially: a single 32-point tile, fewer tiles than workgroups, and more than one
    262 144-point chunk (the second pass reuses stash, slabs and the tile queue) - each against its two ragged halves.  The chunks count KEPT
    points: the two-chunk case runs on field B, which keeps every point of its box (field A keeps about a quarter of its central part)."""
    two = P > 262144
    model, meta = make_model("B" if two else "A")
    f = model.nvfi
    f.requires_grad_(True)
    g = torch.Generator(device="cuda").manual_seed(P)
    mn, mx = f.aabb
    if two:
        pts = torch.rand(P, 3, device="cuda", generator=g) * (mx - mn) + mn
    else:
        pts = torch.rand(P, 3, device="cuda", generator=g) * (mx - mn) * 0.6 + (mn + 0.2 * (mx - mn))      # around the occupied part of field A
    tt = torch.rand(P, 1, device="cuda", generator=g)
    cut = P // 2 - 7

    def term(sl):
        model.zero_grad(set_to_none=True)
        lv = model.get_vel_loss(points=pts[sl], t=tt[sl])
        n = int(f.last_pde_n_kept)
        if n == 0:
            return 0, None
        lv.backward()
        gr = torch.cat([p.grad.reshape(-1).double() for p in f._pde_params()])
        return n, (float(lv.detach()) * n, gr * n)

    n_all, full = term(slice(0, P))
    n_a, a = term(slice(0, cut))
    n_b, b = term(slice(cut, P))
    assert n_all == n_a + n_b and n_all > (2 if P < 100 else 50), (n_all, n_a, n_b)
    if two:
        assert n_all > 262144, n_all       # the second pass does work
    parts = [x for x in (a, b) if x is not None]
    val = sum(x[0] for x in parts)
    grad = sum(x[1] for x in parts)
    np.testing.assert_allclose(full[0], val, rtol=2e-5)
    err = (full[1] - grad).abs().max().item()
    assert err <= 2e-5 * full[1].abs().max().item(), (err, full[1].abs().max().item())


def test_pde_c_abi_with_partial_gradient_sets():
    """nvfi_pde_loss_ex through ctypes with gradient slots left NULL: without the acceleration net's slots the fused adjoint kernel runs its
    first half only (the acceleration net keeps k_pde_jet_bwd's workgroups); without one hidden layer of weight_net the call falls back to the
    unfused adjoint.  The gradients that ARE asked for equal those of the full call."""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    model, meta = make_model("A")
    f = model.nvfi
    g = torch.Generator(device="cuda").manual_seed(11)
    mn, mx = f.aabb
    P = 8192
    pts = (torch.rand(P, 3, device="cuda", generator=g) * (mx - mn) * 0.6 + (mn + 0.2 * (mx - mn))).contiguous()
    tt = torch.rand(P, device="cuda", generator=g).contiguous()
    desc = f._desc()
    nb = C.c_int64(0)
    _lib.check(L.nvfi_pde_workspace_bytes(C.byref(desc), C.c_int64(P), C.byref(nb)))

    def run(drop):
        ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        grads = [torch.zeros_like(p) for p in f._pde_params()]
        G = f._grads_struct_vel(grads)
        if drop == "accel":
            for i in range(6):
                G.aW[i] = None; G.ab[i] = None
        elif drop == "layer2":
            G.vW[2] = None; G.vb[2] = None
        out = torch.zeros(4, device="cuda")
        cnt = torch.zeros(_lib.NCOUNTERS, dtype=torch.int64, device="cuda")
        _lib.check(L.nvfi_pde_loss_ex(C.byref(desc), C.c_int64(P), _lib.ptr(pts), _lib.ptr(tt), C.c_float(1.0), _lib.ptr(out), C.byref(G),
                                      _lib.ptr(ws), C.c_int64(ws.numel()), _lib.ptr(cnt), None, None, C.c_int64(0), None, None))
        torch.cuda.synchronize()
        return out.cpu(), grads

    out0, g0 = run(None)
    assert out0[1] > 100
    for drop, skip in (("accel", range(12, 24)), ("layer2", (4, 5))):
        out1, g1 = run(drop)
        assert torch.equal(out0[:2], out1[:2])
        for k, (a, b) in enumerate(zip(g0, g1)):
            if k in skip:
                assert float(b.abs().max()) == 0.0, (drop, k)
            else:
                scale = float(a.abs().max())
                assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-12, (drop, k, float((a - b).abs().max()), scale)
