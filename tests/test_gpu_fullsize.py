"""BASELINE.json full-size checks (bat 199^3 grid, K=16, 128 samples/ray, 2048 rays, P=262144): the oracle cannot run the
whole step in seconds, so parity is established through (a) the oracle on a 256-ray slice of the same full-size field,
(b) size-independent properties: composite identities, directional finite differences of the loss against the analytic
gradient, PDE-loss linearity in the sample set, ray-sharding invariance."""
import numpy as np
import pytest
import torch

from conftest import assert_grad
from helpers import assert_contract, field_state, named_grads

pytestmark = pytest.mark.gpu


def _field_spec(model):
    from oracle import oracle as orc
    return orc.FieldSpec(*field_state(model))


@pytest.fixture(scope="module")
def scene():
    import bench
    model = bench.build_scene(torch.device("cuda", 0), 199, 128, True)
    o, d = bench.camera_bundle(torch.device("cuda", 0))
    return model, o, d


def _rays(o, d, n, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    idx = torch.randint(0, o.shape[0], (n,), device="cuda", generator=g)
    return o[idx].contiguous(), d[idx].contiguous()


def test_fullsize_slice_matches_oracle(scene):
    """the headline field (BASELINE configs[2]: bat 199^3, K = 16, 128 samples per ray) on a 256-ray train-mode slice at a non-keyframe
    time: rgb / depth / acc under the 1e-4 contract AND the backward - the eleven parameter gradients test_render_vs_oracle_bigger checks
    on the small fields (planes of both branches, basis_mat, render MLP, velocity net through the RK2 adjoint) - against the oracle's"""
    from oracle import oracle as orc
    model, o, d = scene
    f = model.nvfi
    R = 256
    ro, rd = _rays(o, d, R, 1)
    u = torch.rand(R, 1)
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    tg = torch.rand(R, 3, device="cuda", generator=g)
    f.train()
    model.zero_grad(set_to_none=True)
    f.jitter_override = u
    try:
        out = f(19.0 / 60.0, ro, rd, True)
    finally:
        f.jitter_override = None
    (torch.nn.functional.mse_loss(out[0], tg) + 0.01 * out[1].mean()).backward()
    fs = _field_spec(model)
    orc.set_threads(8)
    ref = orc.render(fs, ro.cpu().numpy(), rd.cpu().numpy(), 19.0 / 60.0, u=u.numpy(), train=True, white_bg=True, keep_ctx=True)
    for i, (nm, r) in enumerate((("rgb", ref.rgb), ("depth", ref.depth), ("acc", ref.acc))):     # the 1e-4 contract, flip-band rays counted
        assert_contract(out[i].detach().cpu().numpy(), r, nm, label="hip bat 199^3/128")
    gref = ref.backward(fs, g_rgb=2 * (ref.rgb - tg.cpu().numpy()) / (R * 3), g_depth=np.full(R, 0.01 / R, np.float32))
    ref.free()
    gh = named_grads(model)
    for pn in ("density_plane_space.0", "density_plane_time.2", "app_plane_space.1", "app_plane_time.0", "basis_mat.weight",
               "renderModule.mlp.0.weight", "renderModule.mlp.2.bias", "renderModule.mlp.4.weight",
               "vel_net.weight_net.1.weight", "vel_net.weight_net.4.0.weight", "vel_net.weight_net.7.0.bias"):
        assert_grad(gh[pn], gref[pn], 5e-4, "bat199:" + pn)
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("P", [4096, 32768])
def test_fullsize_pde_slice_matches_oracle(scene, P):
    """the PDE term of the headline field on a slice of collocation points the oracle finishes in seconds: kept set, loss, the forward-mode
    Jacobians of the first kept points (on the intersection of the two kept sets) and the gradients of BOTH velocity nets
    (reference models/nvfi.py:42-84), as test_chessboard_pde_slice_matches_oracle does for configs[3]"""
    from oracle import oracle as orc
    model, o, d = scene
    f = model.nvfi
    fs = _field_spec(model)
    orc.set_threads(8)
    g = torch.Generator(device="cuda"); g.manual_seed(6 + P)
    mn, mx = f.aabb
    pts = torch.rand(P, 3, device="cuda", generator=g) * (mx - mn) + mn
    tt = torch.rand(P, 1, device="cuda", generator=g)
    model.zero_grad(set_to_none=True)
    f.pde_debug = 64
    try:
        lv = model.get_vel_loss(points=pts, t=tt)
    finally:
        f.pde_debug = 0
    ref = orc.pde_loss(fs, pts.cpu().numpy(), tt.cpu().numpy(), n_jac=64)
    kept = f.last_pde_kept.cpu().numpy().astype(bool)
    assert ref["n_kept"] > P // 40, ref["n_kept"]
    assert np.mean(kept != ref["kept"]) < 2e-3                 # alpha within rounding of the 1e-4 threshold may flip
    ours_ids, ref_ids = np.nonzero(kept)[0][:64], np.nonzero(ref["kept"])[0][:64]
    common, io, ir = np.intersect1d(ours_ids, ref_ids, return_indices=True)
    assert len(common) >= 56, len(common)
    np.testing.assert_allclose(f.last_pde_jac.cpu().numpy()[io, :3], ref["jac"][ir, :3], rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(float(lv.detach()), ref["loss"], rtol=5e-4)
    lv.backward()
    gh = named_grads(model)
    n = 0
    for k, r in ref["grads"].items():
        if k.startswith("vel_net.") and r is not None and np.any(r):
            assert_grad(gh[k], r, 1e-3, f"bat199:pde{P}:" + k)
            n += 1
    assert n >= 20, n          # weights and biases of both six-layer nets (the acceleration net's last layers included)
    model.zero_grad(set_to_none=True)


def test_fullsize_composite_identities_and_sharding(scene):
    model, o, d = scene
    f = model.nvfi
    ro, rd = _rays(o, d, 2048, 2)
    f.eval()
    with torch.no_grad():
        rgb, depth, acc, w, _ = f(0.32, ro, rd, True)
        assert torch.allclose(w.sum(-1), acc, rtol=1e-5, atol=1e-6)            # acc = sum of weights
        assert (rgb >= 0).all() and (rgb <= 1).all() and (w >= 0).all() and (acc <= 1 + 1e-5).all()
        assert float(acc.mean()) > 0.02                                         # the blob is visible
        assert int(f.last_counters[0]) > 0.3 * 2048 * 128 and int(f.last_counters[2]) > 1000
        # rays are independent: rendering two shards separately reproduces the joint render bit-for-bit
        a = f(0.32, ro[:1024], rd[:1024], True)
        b = f(0.32, ro[1024:], rd[1024:], True)
        assert torch.equal(torch.cat([a[0], b[0]]), rgb) and torch.equal(torch.cat([a[1], b[1]]), depth)
        # keyframe time == the same time with the velocity switched off (no warp at a keyframe)
        k1 = f(0.30, ro[:512], rd[:512], True)
        f.use_vel = False
        try:
            k2 = f(0.30, ro[:512], rd[:512], True)
        finally:
            f.use_vel = True
        assert torch.allclose(k1[0], k2[0], atol=2e-6)


def test_fullsize_directional_derivative(scene):
    """loss(theta + eps*dir) - loss(theta - eps*dir) ~ 2 eps <grad, dir> for the full step loss (render + PDE)"""
    model, o, d = scene
    f = model.nvfi
    ro, rd = _rays(o, d, 2048, 3)
    u = torch.rand(2048, 1)
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    target = torch.rand(2048, 3, device="cuda", generator=g)
    mn, mx = f.aabb
    pts = torch.rand(262144, 3, device="cuda", generator=g) * (mx - mn) + mn
    tt = torch.rand(262144, 1, device="cuda", generator=g)
    params = {"dps": f.density_plane_space[0], "apt": f.app_plane_time[1], "rW": f.renderModule.mlp[2].weight,
              "vW": f.vel_net.weight_net[4][0].weight, "aW": f.vel_net.a_weight_net[3][0].weight}

    def loss_fn():
        f.train()
        f.jitter_override = u
        try:
            out = f(19.0 / 60.0, ro, rd, True)
        finally:
            f.jitter_override = None
        lv = model.get_vel_loss(points=pts, t=tt)
        return torch.nn.functional.mse_loss(out[0], target) + 0.1 * out[1].mean() * 0.01 + 1.0 * lv

    model.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    assert int(f.last_pde_out[1]) > 1000
    for name, p in params.items():
        gg = torch.Generator(device="cuda"); gg.manual_seed(11)
        direction = torch.randn(p.shape, device="cuda", generator=gg)
        if p.dim() == 4:
            direction = direction.contiguous(memory_format=torch.channels_last)
        analytic = float((p.grad.double() * direction.double()).sum())
        eps = {"dps": 2e-3, "apt": 2e-3, "rW": 1e-3, "vW": 2e-3, "aW": 5e-3}[name]
        with torch.no_grad():
            p.add_(eps * direction); lp = float(loss_fn().double())
            p.add_(-2 * eps * direction); lm = float(loss_fn().double())
            p.add_(eps * direction)
        numeric = (lp - lm) / (2 * eps)
        assert abs(numeric - analytic) <= 0.05 * max(abs(analytic), abs(numeric)) + 2e-5, (name, numeric, analytic)


def test_fullsize_pde_linearity(scene):
    """sum-of-squares bookkeeping: the PDE statistics of two disjoint point sets add up to those of their union"""
    model, o, d = scene
    f = model.nvfi
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    mn, mx = f.aabb
    pts = torch.rand(262144, 3, device="cuda", generator=g) * (mx - mn) + mn
    tt = torch.rand(262144, 1, device="cuda", generator=g)
    with torch.no_grad():
        model.get_vel_loss(points=pts, t=tt); full = f.last_pde_out.double().cpu().numpy()
        model.get_vel_loss(points=pts[:131072], t=tt[:131072]); a = f.last_pde_out.double().cpu().numpy()
        model.get_vel_loss(points=pts[131072:], t=tt[131072:]); b = f.last_pde_out.double().cpu().numpy()
    assert full[1] == a[1] + b[1] and full[1] > 1000
    np.testing.assert_allclose(full[2], a[2] + b[2], rtol=1e-5)
    np.testing.assert_allclose(full[3], a[3] + b[3], rtol=1e-5)
    np.testing.assert_allclose(full[0], 5 * full[2] / full[1] + 0.1 * full[3] / (3 * full[1]), rtol=1e-5)
