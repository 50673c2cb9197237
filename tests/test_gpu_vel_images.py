"""vel_images (csrc/frags.h) is every host entry point's way to the velocity net's weight images: the field's fragment cache when the
descriptor carries one, the call's own workspace otherwise.  tests/test_gpu_round5.py compares cached against uncached renders and
tests/test_gpu_flow.py runs nvfi_render_flow without a cache; these are the calls those two leave open, each run both ways in one process
through the mirror's `_frag_on` toggle on golden field A: the PDE term, a training render at a non-keyframe time, integrate_pos (x6 and
the fp32 MFMA kernel), nvfi_compute_alpha and nvfi_vel_eval.

Bit equality wherever the kernels of the two runs are the same kernels on the same numbers in the same order.  The PDE value is an atomic
sum (rtol 2e-6, the bound of test_fused_launches_are_bit_identical_to_the_round4_launch_chain); weight gradients are sums of the same
products in an order that a device-side queue / atomic cursors decide (relerr < 2e-5, the bound of test_render_mse_backward_matches_autograd
for two summation orders of the same products)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, relerr
from helpers import make_model, named_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    gold = np.load(os.path.join(GOLD, "hotpath.npz"))
    model, meta = make_model("A")
    return model, {k: gold[k] for k in ("A:rays_o", "A:rays_d", "A:train_nonkey:u", "A:train_nonkey:target", "A:pde:points", "A:pde:t")}


def _both(f, run):
    """run() with the fragment cache and without it; the toggle goes back to the environment's choice"""
    from nvfi_amd.models.tensorf_keyframe import _rt
    try:
        _rt(f)["_frag_on"] = True
        a = run()
        assert f._desc().frags, "the cached run had no cache"
        _rt(f)["_frag_on"] = False
        assert not f._desc().frags
        b = run()
    finally:
        _rt(f)["_frag_on"] = None
    return a, b


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), what


def test_pde_call_cached_and_uncached(A):
    model, gold = A
    f = model.nvfi
    pts, tt = _cu(gold["A:pde:points"]), _cu(gold["A:pde:t"])

    def autograd_form():
        f.pde_debug = 4
        try:
            model.zero_grad(set_to_none=True)
            loss = f.pde_loss(pts, tt)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            f.pde_debug = 0
        return dict(kept=f.last_pde_kept.clone(), counters=f.last_pde_counters.clone(), jac=f.last_pde_jac.clone(), out=f.last_pde_out.clone(),
                    grads=[p.grad.detach().clone() for p in f._pde_params()])

    def fused_form():
        grads = [torch.zeros_like(p) for p in f._pde_params()]
        out = f.pde_loss_backward_(pts, tt, weight=0.7, grad_targets=grads)
        torch.cuda.synchronize()
        return dict(counters=f.last_pde_counters.clone(), out=out.clone(), grads=grads)

    for form in (autograd_form, fused_form):
        a, b = _both(f, form)
        for k in ("kept", "counters", "jac"):
            if k in a:
                _same(a[k], b[k], (form.__name__, k))
        assert int(a["counters"][4]) > 256, "the golden points keep more than one workgroup of the jet kernels"
        print(form.__name__, "out", a["out"].tolist(), b["out"].tolist())
        np.testing.assert_allclose(a["out"].cpu().numpy(), b["out"].cpu().numpy(), rtol=2e-6, err_msg=form.__name__)
        assert len(a["grads"]) == 24
        for i, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
            assert float(gb.abs().max()) > 0, (form.__name__, i)
            e = relerr(ga.cpu().numpy(), gb.cpu().numpy())
            print(form.__name__, "grad", i, e)
            assert e < 2e-5, (form.__name__, i, e)


def test_training_render_cached_and_uncached(A):
    model, gold = A
    f = model.nvfi
    o, d, tgt = _cu(gold["A:rays_o"]), _cu(gold["A:rays_d"]), _cu(gold["A:train_nonkey:target"])
    u = _cu(gold["A:train_nonkey:u"]).reshape(-1)
    t = 0.38 * f.tmax / (f.num_keyframes - 1)

    def run():
        model.zero_grad(set_to_none=True)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        f.train()
        try:
            loss, rgb = f.render_mse_backward_(t, o, d, tgt, white_bg=True, jitter=u)
            torch.cuda.synchronize()
        finally:
            f.eval()
        return rgb.clone(), named_grads(model)

    (rgb_a, ga), (rgb_b, gb) = _both(f, run)
    model.zero_grad(set_to_none=True)
    _same(rgb_a, rgb_b, "colours")
    keys = [k for k in ga if k.startswith("vel_net.weight_net.")]
    assert len(keys) == 12
    for k in keys:
        assert np.abs(gb[k]).max() > 0, k
        e = relerr(ga[k], gb[k])
        print(k, e)
        assert e < 2e-5, (k, e)


def _pos_inputs(f, N):
    """N points in the normalised box; even points one RK2 step from their base time, odd points three (dt_max = half a keyframe interval)"""
    g = torch.Generator().manual_seed(1234 + N)
    x = (torch.rand(N, 3, generator=g) * 1.6 - 0.8).cuda()
    ts = f.tmax / (f.num_keyframes - 1)
    base = (torch.randint(0, f.num_keyframes - 2, (N, 1), generator=g).float() * ts).cuda()
    odd = (torch.arange(N, device="cuda") % 2).float()[:, None]
    t = base + (0.3 + 0.9 * odd) * ts
    return x, t, base


# 33: one full 32-point tile and a ragged one; 32 * 4097: one tile past NVFI_X6W_MIN_TILES = 4096, where the one-wave-per-tile x6 kernel takes over
@pytest.mark.parametrize("N", [33, 32 * 4097])
@pytest.mark.parametrize("mode", ["x6", "fp32"])
def test_integrate_pos_cached_and_uncached(A, N, mode):
    model, _ = A
    f = model.nvfi
    x, t, base = _pos_inputs(f, N)
    keep = f.vel_fp16
    try:
        if mode == "fp32":
            f.vel_fp16 = "fp32"      # vel_fp16 bit 3: the fp32 MFMA kernel, the other branch of the warp table
        assert bool(f._desc().vel_fp16 & 8) == (mode == "fp32")
        a, b = _both(f, lambda: f.integrate_pos(x, t, base).clone())
    finally:
        f.vel_fp16 = keep
    assert bool(torch.isfinite(a).all()) and float((a - x).abs().max()) > 0, "the points moved"
    _same(a, b, (N, mode))


def test_compute_alpha_cached_and_uncached(A):
    from nvfi_amd import _lib
    model, _ = A
    f = model.nvfi
    N = 1000
    g = torch.Generator().manual_seed(7)
    xyz = (f.aabb[0].cpu() + torch.rand(N, 3, generator=g) * (f.aabb[1] - f.aabb[0]).cpu()).cuda().contiguous()
    t = 0.38 * f.tmax / (f.num_keyframes - 1)

    def run():
        desc = f._desc()
        nb = C.c_int64(0)
        _lib.check(_lib.lib().nvfi_alpha_workspace_bytes(C.byref(desc), C.c_int64(N), C.byref(nb)))
        ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        alpha = torch.zeros(N, device="cuda")
        _lib.check(_lib.lib().nvfi_compute_alpha(C.byref(desc), C.c_int64(N), _lib.ptr(xyz), C.c_float(float(np.float32(t))), C.c_int(0), C.c_float(f._step_host),
                                                 C.c_int(0), _lib.ptr(alpha), _lib.ptr(ws), C.c_int64(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return alpha

    a, b = _both(f, run)
    assert float(a.max()) > 0, "some of the points are occupied"
    _same(a, b, "alpha")


@pytest.mark.parametrize("gated", [True, False])
def test_vel_eval_cached_and_uncached(A, gated):
    model, _ = A
    f = model.nvfi
    g = torch.Generator().manual_seed(11)
    xt = torch.cat([torch.rand(100, 3, generator=g) * 1.6 - 0.8, torch.rand(100, 1, generator=g) * 2 - 1], 1).cuda()
    a, b = _both(f, lambda: f._vel_eval(xt, gated).clone())
    assert a.shape == (100, 3 if gated else 6) and float(a.abs().max()) > 0
    _same(a, b, gated)
