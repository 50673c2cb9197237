"""Depth loss on the device (csrc/depthloss.hip: nvfi_depth_loss) against the float64 yardstick tests/depth64.py, its autograd wrapper
(utils.compute_depth_loss), the fused driver (render_mse_backward_(..., target_depth=)) on golden field A, and hipGraph capture.

Bound of every kernel comparison, per quantity: 4 x max(ref32_err, 2^-23 x max|quantity in float64|).  ref32_err is the reference's own fp32
error against the yardstick (tests/golden/depthloss.npz: absolute for the loss, relative to depth64.grad_scale for the gradient - max|grad|
of the yardstick, except where the gradient is a cancellation of more than 10 bits of its own terms; 3.2e-7, so the bound is 1.3e-6 of
max|grad|, about 11 fp32 ulp, and fp32 sums or a dropped eps would show); the factor 4 is the
project's allowance for another summation order (test_gpu_charloss.py); the second term is one fp32 ulp of the quantity, so that a luckily
exact reference does not set an impossible bound.  Every comparison prints its error / bound ratio (DESIGN 4.16 records the worst)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import depth64 as d64
from conftest import GOLD, assert_grad, maxrel, relerr
from helpers import assert_contract, make_model, named_grads
from nvfi_amd._lib import NVFI_DEPTH_LDS_MAX

pytestmark = pytest.mark.gpu

CASES = ("distinct", "plateau", "allequal", "signed")
RATIOS = {"loss": 0.0, "grad": 0.0}
_GD = {}


def gd():
    if not _GD:
        _GD["z"] = np.load(os.path.join(GOLD, "depthloss.npz"))
    return _GD["z"]


B = NVFI_DEPTH_LDS_MAX          # the exported boundary between the LDS-resident and the streaming kernel
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2048, B - 1, B, B + 1, 640000]


def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def raw(pred, gt, index=None, skip_holes=False, grad_scale=1.0):
    """the C call through the thin binding: -> (loss float32, grad (n,) numpy, n_counted int); the outputs start from sentinels"""
    from nvfi_amd.utils.evaluation_utils import depth_loss_raw
    p, g = _cu(pred), _cu(gt)
    out = (torch.full((), -7.0, device="cuda"), torch.full((p.numel(),), -7.0, device="cuda"), torch.full((), -7, dtype=torch.int64, device="cuda"))
    loss, grad, cnt = depth_loss_raw(p, g, None if index is None else _cu(index, torch.int64), skip_holes, grad_scale, out=out)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy(), int(cnt)


def compare(label, loss, grad, y):
    z = gd()
    e_l, e_g = d64.errors(loss, grad, y)
    b_l = 4 * max(float(z["ref32_err:loss"]), 2.0 ** -23 * abs(y["loss"]))
    b_g = 4 * max(float(z["ref32_err:grad"]), 2.0 ** -23)
    RATIOS["loss"], RATIOS["grad"] = max(RATIOS["loss"], e_l / b_l), max(RATIOS["grad"], e_g / b_g)
    print(f"[depthloss] {label}: loss err {e_l:.2e} = {e_l / b_l:.3f} x bound, grad err {e_g:.2e} (of max|grad|) = {e_g / b_g:.3f} x bound, "
          f"{e_g / 2.0 ** -23:.2f} fp32 ulp of max|grad|")
    assert e_l <= b_l and e_g <= b_g, (label, e_l, b_l, e_g, b_g)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_the_yardstick(n):
    for ci, case in enumerate(CASES):
        pred, gt = d64.named_case(case, n, 50 * n % 9973 + ci)
        rng = np.random.default_rng(n + 17 * ci)
        # plain
        loss, grad, cnt = raw(pred, gt)
        y = d64.depth64(pred, gt)
        assert cnt == n
        compare(f"n={n} {case}", loss, grad, y)
        if n == 1:
            assert float(loss) == 0.0 and float(grad[0]) == 0.0
        # two calls: the same bits
        loss2, grad2, _ = raw(pred, gt)
        assert loss.tobytes() == loss2.tobytes() and grad.tobytes() == grad2.tobytes(), (n, case)
        # holes: targets 0, -1, inf, NaN at a seeded third of the entries
        gt_h = gt.copy()
        holes = rng.permutation(n)[: n // 3]
        gt_h[holes] = np.array([0.0, -1.0, np.inf, np.nan], np.float32)[np.arange(len(holes)) % 4]
        if case == "signed":
            gt_h = np.where(np.isin(np.arange(n), holes), gt_h, np.abs(gt_h) + np.float32(0.5)).astype(np.float32)   # the counted targets must be > 0
        loss, grad, cnt = raw(pred, gt_h, skip_holes=True)
        y = d64.depth64(pred, gt_h, skip_holes=True)
        assert cnt == y["n_counted"] == n - len(holes)
        compare(f"n={n} {case} holes", loss, grad, y)
        assert not grad[holes].any()
        # gather: repeated and permuted indices into a longer image
        image = rng.uniform(1.0, 8.0, n + 37).astype(np.float32) if case != "signed" else rng.uniform(-4.0, 4.0, n + 37).astype(np.float32)
        index = rng.integers(0, image.size, n)
        if n > 2:
            index[1] = index[0]
            index[n // 2:] = rng.permutation(np.arange(image.size))[: n - n // 2]
        loss, grad, cnt = raw(pred, image, index=index)
        compare(f"n={n} {case} gather", loss, grad, d64.depth64(pred, image, gt_index=index))
        lossg, gradg, _ = raw(pred, image[index])
        assert loss.tobytes() == lossg.tobytes() and grad.tobytes() == gradg.tobytes()
    print(f"[depthloss] worst error / bound so far: loss {RATIOS['loss']:.3f}, grad {RATIOS['grad']:.3f}")


def test_plateau_gradient_is_split_equally():
    """[5,2,2,2,1]: torch autograd gives the median's gradient to the three 2s in thirds; entries that tie AND share a target get the same bits"""
    pred = np.array([5, 2, 2, 2, 1], np.float32)
    gt = np.array([3, 4, 4, 4, 9], np.float32)
    loss, grad, _ = raw(pred, gt)
    assert grad[1] == grad[2] == grad[3]
    compare("thirds", loss, grad, d64.depth64(pred, gt))
    n = 2048
    pred, gt = d64.named_case("plateau", n, 3)
    gt[pred == 8.0] = np.float32(2.5)
    loss, grad, _ = raw(pred, gt)
    assert np.unique(grad[pred == 8.0]).size == 1 and (pred == 8.0).sum() > n // 2
    compare("plateau, one target", loss, grad, d64.depth64(pred, gt))


def test_grad_scale_scales_the_gradient_only():
    pred, gt = d64.named_case("plateau", 1025, 9)
    l1, g1, _ = raw(pred, gt)
    l2, g2, _ = raw(pred, gt, grad_scale=0.25)       # a power of two: exact
    assert l1.tobytes() == l2.tobytes() and np.array_equal(g2, 0.25 * g1)


@pytest.mark.parametrize("n", [65, 2048, 16385])
def test_nan_all_holes_and_refusals(n):
    from nvfi_amd import _lib
    pred, gt = d64.named_case("distinct", n, 11)
    # one NaN among the counted entries: NaN loss, every counted gradient NaN, the call returns normally
    for where in ("pred", "gt"):
        p, g = pred.copy(), gt.copy()
        (p if where == "pred" else g)[n // 3] = np.nan
        loss, grad, cnt = raw(p, g)
        assert np.isnan(loss) and np.isnan(grad).all() and cnt == n, where
    # ... and with holes around it: uncounted entries keep an exact 0
    p, g = pred.copy(), gt.copy()
    p[5] = np.nan
    g[:3] = 0.0
    loss, grad, cnt = raw(p, g, skip_holes=True)
    assert np.isnan(loss) and np.isnan(grad[3:]).all() and not grad[:3].any() and cnt == n - 3
    # a NaN at a hole does not count
    p = pred.copy()
    p[1] = np.nan
    loss, grad, cnt = raw(p, g, skip_holes=True)
    assert np.isfinite(loss) and np.isfinite(grad).all() and grad[1] == 0.0
    # all holes
    loss, grad, cnt = raw(pred, np.zeros(n, np.float32), skip_holes=True)
    assert float(loss) == 0.0 and not grad.any() and cnt == 0
    # refusals: an error code, nothing launched (the sentinels stay)
    L = _lib.lib()
    p, g = _cu(pred), _cu(gt)
    loss_t, grad_t = torch.full((), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad_n in (0, -1, (1 << 22) + 1):
        rc = L.nvfi_depth_loss(C.c_int64(bad_n), _lib.ptr(p), _lib.ptr(g), None, C.c_int(0), C.c_float(1.0), _lib.ptr(loss_t), _lib.ptr(grad_t), None, st)
        assert rc != 0 and b"nvfi_depth_loss" in L.nvfi_last_error(), bad_n
    assert L.nvfi_depth_loss(C.c_int64(n), None, _lib.ptr(g), None, C.c_int(0), C.c_float(1.0), _lib.ptr(loss_t), _lib.ptr(grad_t), None, st) != 0
    assert L.nvfi_depth_loss(C.c_int64(n), _lib.ptr(p), _lib.ptr(g), None, C.c_int(0), C.c_float(1.0), _lib.ptr(loss_t), None, None, st) != 0
    torch.cuda.synchronize()
    assert float(loss_t) == -7.0 and bool((grad_t == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- autograd wrapper
def test_autograd_wrapper_equals_the_raw_call():
    from nvfi_amd import _lib
    from nvfi_amd.utils import compute_depth_loss
    pred, gt = d64.named_case("plateau", 2049, 21)
    gt[::7] = 0.0
    for skip in (False, True):
        l0, g0, _ = raw(pred, gt, skip_holes=skip)
        p = _cu(pred).reshape(3, 683).requires_grad_(True)          # any shape, flattened
        loss = compute_depth_loss(p, _cu(gt).reshape(683, 3), skip_holes=skip)
        assert loss.dim() == 0 and loss.requires_grad and loss.detach().cpu().numpy().tobytes() == l0.tobytes()
        (0.3 * loss).backward()
        assert p.grad.shape == p.shape
        assert np.array_equal(p.grad.cpu().numpy().ravel(), np.float32(0.3) * g0)       # that one multiply
    with pytest.raises(NotImplementedError):
        compute_depth_loss(_cu(pred), _cu(gt).requires_grad_(True))
    with pytest.raises(_lib.NvfiError):
        compute_depth_loss(torch.from_numpy(pred), torch.from_numpy(gt))
    with pytest.raises(_lib.NvfiError):
        compute_depth_loss(_cu(pred), torch.from_numpy(gt))
    # the thin binding checks the gather's indices before it launches (the kernel does not)
    from nvfi_amd.utils.evaluation_utils import depth_loss_raw
    for bad in (-1, 2049):
        idx = torch.arange(2049, device="cuda")
        idx[100] = bad
        with pytest.raises(IndexError):
            depth_loss_raw(_cu(pred), _cu(gt), idx)


# ---------------------------------------------------------------------------------------------------------------- end to end, field A
class E2E:
    pass


_E2E = {}


def e2e():
    """model A, golden rays / jitter / targets and ONE training render with its graph kept: built once, shared"""
    if "c" in _E2E:
        return _E2E["c"]
    from nvfi_amd.models import Renderer, Ray
    z, hot = gd(), np.load(os.path.join(GOLD, "hotpath.npz"))
    c = E2E()
    c.model, c.meta = make_model("A")
    c.f = c.model.nvfi
    c.o, c.d = _cu(hot["A:rays_o"]), _cu(hot["A:rays_d"])
    c.t, c.w = float(z["e2e:t"]), float(z["e2e:w"])
    c.target = _cu(hot["A:train_nonkey:target"])
    c.u = torch.from_numpy(hot["A:train_nonkey:u"].copy())
    c.gt = z["e2e:gt"]
    c.model.zero_grad(set_to_none=True)
    torch.manual_seed(21)        # same CPU-generator stream as the reference: jitter, then the white coin (test_gpu_parity.test_render_train_grads)
    out = Renderer(c.model, 0, 0, 2048).render(c.t, Ray(c.o, c.d, 0, 1), white_background=bool(c.meta["white_background"]), mode="train")
    c.rgb, c.depth = out[0], out[1]
    _E2E["c"] = c
    return c


def test_e2e_depth_meets_the_contract_and_the_kernel_the_yardstick():
    c, z = e2e(), gd()
    depth = c.depth.detach().cpu().numpy().reshape(-1)
    assert_contract(depth, z["e2e:depth"], "depth", label="hip e2e")                       # (a)
    loss, grad, cnt = raw(depth, c.gt, skip_holes=True)                                    # (b) at the GPU's own depth
    assert cnt == z["e2e:subset"].size
    compare("e2e field A", loss, grad, d64.depth64(depth, c.gt, skip_holes=True))


def test_e2e_parameter_gradients_under_the_golden_depth_gradient():
    """(c) the g_depth path of the render backward with a real depth-loss gradient: independent of how the loss conditions the depth"""
    c, z = e2e(), gd()
    c.model.zero_grad(set_to_none=True)
    torch.autograd.backward([c.rgb, c.depth], [_cu(z["e2e:g_rgb"]), _cu(z["e2e:g_depth"]).reshape(c.depth.shape)])
    g = named_grads(c.model)
    checked = 0
    for k in z.files:
        pre = "e2e:grad:nvfi."
        if not k.startswith(pre):
            continue
        pn, ref = k[len(pre):], z[k]
        if pn == "basis_mat_density.weight":
            continue
        if ref.size == 0:
            assert g[pn] is None or not np.any(g[pn]), pn
            continue
        assert_grad(g[pn], ref, 5e-4, pn)
        checked += 1
    assert checked >= 22
    c.model.zero_grad(set_to_none=True)
    _E2E.clear()                   # the graph is spent


def test_e2e_fused_route_equals_the_drop_in_route():
    from nvfi_amd.utils import compute_depth_loss
    c = e2e()
    model, f, w = c.model, c.f, c.w
    gt = _cu(c.gt)
    uj = c.u.cuda().reshape(-1)
    # drop-in: autograd, mse + w * compute_depth_loss(depth, gt)
    model.zero_grad(set_to_none=True)
    f.train()
    f.jitter_override = c.u
    try:
        out = f(c.t, c.o, c.d, True)
    finally:
        f.jitter_override = None
    mse = torch.nn.functional.mse_loss(out[0], c.target)
    dl = compute_depth_loss(out[1], gt, skip_holes=True)
    (mse + w * dl).backward()
    ref_mse, ref_dl, ref_rgb, ref_g = float(mse.detach()), dl.detach().clone(), out[0].detach().clone(), named_grads(model)

    def fused(**kw):
        model.zero_grad(set_to_none=True)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        f.train()
        return f.render_mse_backward_(c.t, c.o, c.d, c.target, white_bg=True, jitter=uj, **kw)

    # (d) fused: both loss terms and every gradient (comparison and tolerance of test_render_mse_backward_matches_autograd)
    res = fused(target_depth=gt, depth_weight=w, skip_holes=True)
    assert len(res) == 3
    loss, rgb, dloss = res
    assert torch.equal(rgb, ref_rgb)
    assert abs(float(loss) - ref_mse) <= 2e-6 * abs(ref_mse)
    assert abs(float(dloss) - float(ref_dl)) <= 2e-6 * abs(float(ref_dl)) and dloss.dim() == 0
    g = named_grads(model)
    n = 0
    for k, r in ref_g.items():
        if r is None:
            continue
        assert relerr(g[k], r) < 2e-5, k
        n += 1
    assert n >= 19
    # the depth term reaches the gradients: without it they differ
    res0 = fused()
    assert len(res0) == 2                                                                   # (e) two values, as before
    g0 = named_grads(model)
    assert maxrel(g0["density_plane_space.0"], ref_g["density_plane_space.0"]) > 1e-3
    # loss_scale scales the depth gradient too
    fused(target_depth=gt, depth_weight=w, skip_holes=True, loss_scale=0.25)
    assert relerr(named_grads(model)["density_plane_space.0"], 0.25 * ref_g["density_plane_space.0"]) < 2e-5
    # (f) a depth image + depth_index (what nvfi_draw_batch writes as pixel_ids) against the gathered vector: the same bits
    rng = np.random.default_rng(8)
    R = gt.numel()
    ids = rng.permutation(4 * R)[:R]
    image = rng.uniform(1.0, 6.0, 4 * R).astype(np.float32)
    image[ids] = c.gt
    dl_img = fused(target_depth=_cu(image), depth_index=_cu(ids, torch.int64), depth_weight=w, skip_holes=True)[2].clone()
    g_img = named_grads(model)
    dl_vec = fused(target_depth=gt, depth_weight=w, skip_holes=True)[2].clone()
    assert dl_img.cpu().numpy().tobytes() == dl_vec.cpu().numpy().tobytes() == dloss.cpu().numpy().tobytes()
    assert relerr(g_img["density_plane_space.0"], ref_g["density_plane_space.0"]) < 2e-5
    # arguments that cannot be right are refused before anything is launched
    with pytest.raises(ValueError):
        fused(target_depth=gt[:-1])
    with pytest.raises(ValueError):
        fused(target_depth=_cu(image), depth_index=_cu(ids[:-1], torch.int64))
    bad = ids.copy()
    bad[7] = image.size
    with pytest.raises(IndexError):
        fused(target_depth=_cu(image), depth_index=_cu(bad, torch.int64), check_depth_index=True)
    model.zero_grad(set_to_none=True)


def test_evaluation_reports_the_depth_loss_per_frame():
    """render_test_evaluation(gt_depths=): the same kernel per frame, holes skipped"""
    from nvfi_amd.models import Renderer, Camera
    from nvfi_amd.utils import compute_depth_loss, render_test_evaluation
    c = e2e()
    H = W = 12
    near, far = [float(v) for v in c.f.near_far]
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, 4.0])
    ren = Renderer(c.model, 0, 0, 2048)
    rng = np.random.default_rng(2)
    gts = rng.uniform(near, far, (2, H, W)).astype(np.float32)
    gts[0, :2] = 0.0
    res = render_test_evaluation(c.model, ren, [pose.numpy()] * 2, [0.0, c.t], None, H, W, 20.0, near, far, update_alpha_mask=False, gt_depths=gts)
    assert len(res["depth_loss"]) == 2 and all(np.isfinite(res["depth_loss"])) and res["mean_depth_loss"] == sum(res["depth_loss"]) / 2
    with torch.no_grad():
        cam = Camera(pose.cuda(), H, W, 20.0, None, near, far)
        depth = ren.render(c.t, cam.rays.to("cuda"), white_background=True, mode="test")[1]
        assert float(compute_depth_loss(depth, _cu(gts[1]), skip_holes=True)) == res["depth_loss"][1]
    assert "depth_loss" not in render_test_evaluation(c.model, ren, [pose.numpy()], [0.0], None, H, W, 20.0, near, far, update_alpha_mask=False)


# ---------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("n", [2048, 16385])
def test_graph_capture_and_replay(n):
    from nvfi_amd.utils.evaluation_utils import depth_loss_raw
    pa, ga = d64.named_case("plateau", n, 1)
    pb, gb = d64.named_case("distinct", n, 2)
    gb[::5] = 0.0
    p, g = _cu(pa), _cu(ga)
    out = (torch.zeros((), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"))
    depth_loss_raw(p, g, None, True, 1.0, out=out)          # (the launcher's per-device set-up happens outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        depth_loss_raw(p, g, None, True, 1.0, out=out)
    torch.cuda.current_stream().wait_stream(cap)
    p.copy_(_cu(pb))
    g.copy_(_cu(gb))
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    loss, grad, cnt = raw(pb, gb, skip_holes=True)
    assert out[0].cpu().numpy().tobytes() == loss.tobytes() and out[1].cpu().numpy().tobytes() == grad.tobytes() and int(out[2]) == cnt
    assert cnt == n - len(gb[::5])
