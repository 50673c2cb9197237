"""CPU checks of the float64 yardstick tests/optim64.py (no GPU): plane regularisers, Adam, MSE.

  regs  against the reference's own fp32 outputs, the goldens "{A,B}:regs:{L1,TVd,TVa}" of tests/golden/hotpath.npz.  Bound = 4 x the measured
        distance of the golden from the float64 yardstick (relative), worst of the two fields:
            L1 7.23e-08 (field A), TVd 7.48e-08 (field B), TVa 7.41e-08 (field A)
        (the goldens are stored in fp32: these distances are about half an fp32 spacing, and the yardstick evaluated in float32 gives the same fp32
        number in five of the six cases.)
  regs  against torch autograd in float64 of the product's torch-ops path (regs_torch_ops on a CPU .double() copy of fields A and B): the
        three values and all nine weighted gradients at rounding level (<= 1e-12 relative).
  adam  against torch.optim.Adam in float64 over 7 steps with a learning rate that changes every step, and mse against F.mse_loss in float64:
        <= 1e-12 relative.  (Betas, eps and lr are given as fp32-representable numbers: the yardstick rounds them to fp32 as the C ABI does,
        torch.optim.Adam takes the doubles.)
The mutations that the GPU tests rely on are checked here to change what they are meant to change."""
import numpy as np
import pytest
import torch

import optim64 as o64
from helpers import load_meta, make_model

KINDS = ["A", "B"]
MEASURED = {"L1": 7.23e-8, "TVd": 7.48e-8, "TVa": 7.41e-8}      # |golden - yardstick64| / |yardstick64|, worst of fields A and B
BOUND = {q: 4.0 * e for q, e in MEASURED.items()}
W3 = (8e-4, 0.7, 1.3)
PLANES = [f"nvfi.{n}.{i}" for n in ("density_plane_space", "density_plane_time", "app_plane_space") for i in range(3)]


def fixture_planes(kind):
    meta, sd = load_meta(kind)
    return [np.asarray(sd[k], np.float32) for k in PLANES], int(meta["num_keyframes"])


@pytest.mark.parametrize("kind", KINDS)
def test_regs_match_the_reference_goldens(gold, kind):
    planes, K = fixture_planes(kind)
    vals, _ = o64.regs(planes, K, W3)
    v32, _ = o64.regs(planes, K, W3, dtype=np.float32)
    for q, v, v3 in zip(("L1", "TVd", "TVa"), vals, v32):
        g = float(gold[f"{kind}:regs:{q}"][0])
        e = abs(g - float(v)) / abs(float(v))
        print(f"[optim64] {kind}: {q}: golden against float64 {e:.2e} (bound {BOUND[q]:.2e}), float32 evaluation against float64 {o64.err(v3, v):.2e}")
        assert e <= BOUND[q], (kind, q, e)


@pytest.mark.parametrize("kind", KINDS)
def test_regs_match_torch_autograd_in_float64(kind):
    from nvfi_amd.utils import TVLoss
    model, _ = make_model(kind, device="cpu")
    model = model.double()
    f = model.nvfi
    f.regs_torch_ops = True
    tv = TVLoss()
    model.zero_grad(set_to_none=True)
    vals_t = [f.density_L1(), f.TV_loss_density(tv), f.TV_loss_app(tv)]
    sum(float(np.float32(w)) * v for w, v in zip(W3, vals_t)).backward()
    planes, K = fixture_planes(kind)
    vals, grads = o64.regs(planes, K, W3)
    for q, a, b in zip(("L1", "TVd", "TVa"), vals, vals_t):
        assert o64.err(a, b.item()) <= 1e-12, (kind, q)
    ps = list(f.density_plane_space) + list(f.density_plane_time) + list(f.app_plane_space)
    for k, (g, p) in enumerate(zip(grads, ps)):
        assert np.array_equal(p.detach().numpy(), planes[k].astype(np.float64))
        e = o64.err(g, p.grad.numpy())
        assert e <= 1e-12, (kind, PLANES[k], e)
    for p in f.app_plane_time:
        assert p.grad is None


def test_regs_edges_and_mutations():
    """K = 1 leaves the time planes out of TVd; exact 0 / 1 entries give a zero L1 gradient; accumulation adds to g0; each mutation moves
    exactly the quantities it is meant to move"""
    rng = np.random.default_rng(0)
    G, Cd, Ca = (7, 5, 9), 8, 12

    def mk(K):
        sp = lambda C, i: rng.standard_normal((1, C, G[o64.SPACE_MODES[i][1]], G[o64.SPACE_MODES[i][0]])).astype(np.float32)
        return [sp(Cd, i) for i in range(3)] + [1 + 0.3 * rng.standard_normal((1, Cd, K, G[o64.TIME_AXIS[i]])).astype(np.float32) for i in range(3)] + \
               [sp(Ca, i) for i in range(3)]

    planes = mk(2)
    planes[0][0, 1, 2, 3] = 0.0
    planes[3][0, 1, 1, 3] = 1.0
    vals, grads = o64.regs(planes, 2, (1.0, 0.0, 0.0))
    assert grads[0][0, 1, 2, 3] == 0 and grads[3][0, 1, 1, 3] == 0 and np.count_nonzero(grads[0]) == grads[0].size - 1
    assert all(not g.any() for g in grads[6:])
    g0 = [rng.standard_normal(p.shape).astype(np.float32) for p in planes]
    _, acc = o64.regs(planes, 2, W3, g0=g0)
    _, g = o64.regs(planes, 2, W3)
    assert all(np.allclose(a - n, b, rtol=0, atol=1e-15) for a, n, b in zip(acc, g0, g))
    p1 = mk(1)
    v1, gr1 = o64.regs(p1, 1, (0.0, 1.0, 0.0))
    vs, _ = o64.regs(p1[:3] + p1[:3] + p1[6:], 1, (0.0, 1.0, 0.0))      # (any time planes: they do not enter)
    assert v1[1] == vs[1] and all(not g.any() for g in gr1[3:6])
    # mutations
    vb, gb = o64.regs(planes, 2, W3)
    for mut, moved_vals, moved_grads in (("last_row", {2}, {6}), ("no_t3", {1}, {3, 4, 5}), ("last4", {0}, {0})):
        vm, gm = o64.regs(planes, 2, W3, mutate=mut)
        assert {i for i in range(3) if vm[i] != vb[i]} == moved_vals, mut
        assert {k for k in range(9) if not np.array_equal(gm[k], gb[k])} == moved_grads, mut


def test_adam_matches_torch_in_float64():
    torch.manual_seed(0)
    b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.99)), float(np.float32(1e-8))
    shapes = [(3,), (5, 7), (1, 4, 3, 2)]
    p0 = [torch.randn(*s).float() for s in shapes]
    ps = [torch.nn.Parameter(p.double().clone()) for p in p0]
    lrs0 = [float(np.float32(0.02)), float(np.float32(1e-3)), float(np.float32(3e-4))]
    opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ps, lrs0)], betas=(b1, b2), eps=eps)
    gs, lrs = [[] for _ in ps], [[] for _ in ps]
    for it in range(7):
        for k, p in enumerate(ps):
            g = (torch.randn_like(p0[k]) * 10.0 ** (it % 3 - 1)).float()
            gs[k].append(g.numpy())
            p.grad = g.double()
            lrs[k].append(opt.param_groups[k]["lr"])
        opt.step()
        for grp in opt.param_groups:
            grp["lr"] = float(np.float32(grp["lr"] * 0.7))
    for k, p in enumerate(ps):
        yp, ym, yv = o64.adam(p0[k].numpy(), gs[k], lrs[k], b1, b2, eps)
        st = opt.state[p]
        for name, a, b in (("p", yp, p.detach()), ("exp_avg", ym, st["exp_avg"]), ("exp_avg_sq", yv, st["exp_avg_sq"])):
            e = o64.err(a, b.numpy())
            assert e <= 1e-12, (k, name, e)
    # continuing from a state: steps 4..7 from the state after step 3 give the same result
    k = 1
    p3, m3, v3 = o64.adam(p0[k].numpy(), gs[k][:3], lrs[k][:3], b1, b2, eps, dtype=np.float32)
    a = o64.adam(p3, gs[k][3:], lrs[k][3:], b1, b2, eps, m0=m3, v0=v3, t0=3, dtype=np.float32)
    b = o64.adam(p0[k].numpy(), gs[k], lrs[k], b1, b2, eps, dtype=np.float32)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(x.dtype == np.float32 for x in b)


@pytest.mark.parametrize("n", [1, 65, 6144])
def test_mse_matches_torch_in_float64(n):
    rng = np.random.default_rng(n)
    x, y = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    tx = torch.from_numpy(x).double().requires_grad_()
    loss = torch.nn.functional.mse_loss(tx, torch.from_numpy(y).double())
    loss.backward()
    v, g = o64.mse(x, y)
    assert o64.err(v, loss.item()) <= 1e-12 and o64.err(g, tx.grad.numpy()) <= 1e-12
    if n > 1:
        vm, gm = o64.mse(x, y, mutate="n-1")
        assert abs(vm / v - n / (n - 1)) <= 1e-12 and o64.err(gm, g * n / (n - 1)) <= 1e-12


def test_bound_helpers():
    assert o64.err(np.float32(1.5), 1.0) == 0.5 and o64.err([1.0, 2.0], [1.0, 4.0]) == max(0.5, 2.0 / np.sqrt(17.0))
    assert o64.ulp_floor(np.array([1.0, -3.0])) == 4 * 2.0 ** -22 / 3.0
    assert o64.bound(np.array([1.0, 2.0]), np.array([1.0, 2.0])) == o64.ulp_floor(np.array([2.0]))       # exact float32 evaluation: the floor
    assert o64.bound(np.array([1.0, 2.1]), np.array([1.0, 2.0])) == 4 * o64.err([1.0, 2.1], [1.0, 2.0])
