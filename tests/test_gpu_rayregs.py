"""Distortion loss on ray weights on the GPU (csrc/raydist.hip, nvfi_ray_distortion): the kernel against the float64 yardstick
(tests/raydist64.py: direct double sum over explicit midpoints) at every chunk / workgroup edge, bit-repeatability and hipGraph capture,
refusals, the autograd wrapper (utils.distortion_loss) and the fused driver (render_mse_backward_(..., distortion_weight=)) on golden field A
against the same loss in fp32 torch ops, and the evaluation driver's floater maps.

Bound: max(3 x fp32 floor of the yardstick's own sums, 1e-5) per tensor = 1e-5 (floors 1.2e-7 / 2.0e-7 / 1.7e-7, tests/golden/rayregs.npz).
The blind-spot checks of these shapes (last sample at S = 65, last ray at R = 5, samples 63 / 64 at S = 129) are asserted on the CPU in
tests/test_rayregs_golden.py::test_blind_spot_*, on the first five rows of the 257-ray arrays built here (a case's rows do not depend on its
ray count).  Every comparison prints error / bound; the worst per quantity is printed when the module's tests are done."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raydist64 as r64
from conftest import GOLD, maxrel, relerr
from helpers import make_model, named_grads

pytestmark = pytest.mark.gpu

S_ALL = (1, 2, 63, 64, 65, 127, 128, 129, 686, 1024)
R_ALL = (1, 3, 4, 5, 257)
SENT = 7.5            # outputs start from this value: an entry the kernel does not write stays visible
WORST = {"loss": 0.0, "grad": 0.0, "per_ray": 0.0}


def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


_GR = {}


def gr():
    if not _GR:
        _GR["z"] = np.load(os.path.join(GOLD, "rayregs.npz"))
    return _GR["z"]


def bounds():
    return {k: r64.bound(float(gr()["ref32_err:" + k])) for k in ("loss", "grad", "per_ray")}


def raw(w, delta, R=None, want=("loss", "grad", "per_ray"), grad_scale=1.0, grad_scale_dev=None):
    """one nvfi_ray_distortion call on the first R rays of the device tensor w, outputs from sentinels -> dict of numpy arrays"""
    from nvfi_amd.utils import distortion_loss_raw
    w = w if R is None else w[:R]
    R, S = w.shape
    out = (torch.full((), SENT, device="cuda") if "loss" in want else None,
           torch.full((R, S), SENT, device="cuda") if "grad" in want else None,
           torch.full((R,), SENT, device="cuda") if "per_ray" in want else None)
    distortion_loss_raw(w, delta, grad_scale=grad_scale, grad_scale_dev=grad_scale_dev, out=out)
    torch.cuda.synchronize()
    return {k: (None if o is None else o.cpu().numpy()) for k, o in zip(("loss", "grad", "per_ray"), out)}


def compare(label, got, y):
    b = bounds()
    e = dict(zip(("loss", "grad", "per_ray"), r64.errors(got["loss"], got["grad"], got["per_ray"], y)))
    if y["loss"] == 0.0:
        assert float(got["loss"]) == 0.0
        e["loss"] = 0.0
    print(f"{label}: " + ", ".join(f"{k} {e[k]:.2e} = {e[k] / b[k]:.3f} x bound" for k in e))
    for k in e:
        WORST[k] = max(WORST[k], e[k] / b[k])
        assert e[k] <= b[k], (label, k, e[k], b[k])
    assert got["grad"].dtype == np.float32 and not (got["grad"] == SENT).any() and not (got["per_ray"] == SENT).any()


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """after the module's tests: the worst error / bound per quantity of the comparisons that ran (each of them asserted its own), for DESIGN 4.18"""
    yield
    print("\nworst error / bound:", ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


# ---------------------------------------------------------------------------------------------------------------- kernel against the yardstick
@pytest.mark.parametrize("S", S_ALL)
def test_kernel_matches_the_yardstick(S):
    """every synthetic case at S x every R: the 257-ray input repeats PERIOD distinct rays, the yardstick runs once on those and serves every R
    (per-ray values are independent; loss = mean of the first R, gradient rows / R).  NULL outputs and both gradient scales at R = 5."""
    Rmax = max(R_ALL)
    for case in r64.CASES:
        seed = r64.CASES.index(case) * 100 + S
        wn = r64.named_case(case, Rmax, S, seed)
        t_min, u, step = r64.geometry(Rmax, S, seed)
        delta = r64.delta_of(step)
        D, G = r64.tiled(wn, t_min, step, u, Rmax)
        w = _cu(wn)
        for R in R_ALL:
            got = raw(w, delta, R)
            compare(f"{case} S={S} R={R}", got, r64.assemble(D, G, R))
            if case == "zeros" and R >= 3:                  # ray 1 is all zero: value and gradient row exactly 0
                assert got["per_ray"][1] == 0.0 and not got["grad"][1].any()
            if case == "spike":                             # D_r = delta w^2 / 3: one rounding to fp32; the gradient at the spike is (2/3) w delta / R
                d32 = np.float64(np.float32(delta))
                wmax = wn[:R].max(1).astype(np.float64)
                assert np.array_equal(got["per_ray"], (d32 * (wmax * wmax / 3.0)).astype(np.float32))
                k23 = np.float32(d32 * (1.0 / R) * 2.0 / 3.0)
                at = wn[:R].argmax(1)
                assert np.array_equal(got["grad"][np.arange(R), at], k23 * wn[:R].max(1))
            if R != 5:
                continue
            for drop in ("loss", "per_ray", "grad"):        # an output left out (NULL): the others do not change by a bit
                part = raw(w, delta, R, want=tuple(k for k in ("loss", "grad", "per_ray") if k != drop))
                assert part[drop] is None
                for k in part:
                    if k != drop:
                        assert part[k].tobytes() == got[k].tobytes(), (case, S, drop, k)
            a = raw(w, delta, R, grad_scale=0.25)
            b = raw(w, delta, R, grad_scale_dev=torch.full((1,), 0.5, device="cuda"))
            assert a["loss"].tobytes() == b["loss"].tobytes() == got["loss"].tobytes() and a["per_ray"].tobytes() == got["per_ray"].tobytes()
            y = r64.assemble(D, G, R)
            for g, s in ((a["grad"], 0.25), (b["grad"], 0.5)):
                e = r64._rel(g, s * y["grad"])
                assert e <= bounds()["grad"], (case, S, s, e)
                assert np.array_equal(g, np.float32(s) * got["grad"])          # powers of two: the same bits, scaled


@pytest.mark.parametrize("kind", ["A", "B"])
def test_kernel_on_the_golden_weight_maps(gold, kind):
    """the (256, 59) and (256, 56) weight maps of a training render of the golden fields, delta = 1 / S"""
    wn, t_min, u, step = r64.golden_map(gold, kind)
    R, S = wn.shape
    delta = r64.delta_of(step)
    assert delta == 1.0 / S and wn.shape == ((256, 59) if kind == "A" else (256, 56))
    D, G = r64.rays(wn, t_min, step, u)
    w = _cu(wn)
    for R in (5, 256):
        compare(f"map {kind} R={R}", raw(w, delta, R), r64.assemble(D, G, R))


# ---------------------------------------------------------------------------------------------------------------- repeats, capture, refusals
def _big_case():
    S, R = 686, 257
    wn = r64.named_case("two_surfaces", R, S, 11)
    wn[13:] = np.random.default_rng(5).permutation(wn[13:].ravel()).reshape(R - 13, S)         # no two rays alike
    return wn, r64.delta_of(r64.geometry(R, S, 11)[2])


def test_two_calls_give_the_same_bits():
    wn, delta = _big_case()
    w = _cu(wn)
    a, b = raw(w, delta), raw(w, delta)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_graph_capture_and_replay():
    from nvfi_amd.utils.ray_regs import distortion_loss_raw, distortion_workspace
    wn, delta = _big_case()
    R, S = wn.shape
    eager = raw(_cu(wn), delta)
    w = torch.zeros(R, S, device="cuda")
    ws = distortion_workspace(R, "cuda")
    out = (torch.zeros((), device="cuda"), torch.zeros(R, S, device="cuda"), torch.zeros(R, device="cuda"))
    distortion_loss_raw(w, delta, out=out, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=cap):
        distortion_loss_raw(w, delta, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(cap)
    w.copy_(_cu(wn))
    for rep in range(2):
        for o in out:
            o.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        for k, o in zip(("loss", "grad", "per_ray"), out):
            assert o.cpu().numpy().tobytes() == eager[k].tobytes(), (rep, k)


def test_refusals():
    from nvfi_amd import _lib
    from nvfi_amd.utils.ray_regs import distortion_loss_raw, distortion_workspace
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # R = 0: loss = 0, nothing else
    loss = torch.full((), SENT, device="cuda")
    distortion_loss_raw(torch.empty(0, 8, device="cuda"), 0.1, out=(loss, None, None))
    assert float(loss) == 0.0
    # a workspace one byte short: error 4 before any launch
    R, S = 5, 65
    w = _cu(r64.named_case("fog", R, S, 1))
    g = torch.full((R, S), SENT, device="cuda")
    ws = distortion_workspace(R, "cuda")
    loss.fill_(SENT)
    args = (C.c_int64(R), C.c_int(S), _lib.ptr(w), C.c_float(0.1), C.c_float(1.0), None, _lib.ptr(loss), None, _lib.ptr(g), _lib.ptr(ws))
    assert L.nvfi_ray_distortion(*args, C.c_int64(ws.numel() - 1), st) == 4
    assert b"workspace" in L.nvfi_last_error()
    assert L.nvfi_ray_distortion(*args[:9], None, C.c_int64(ws.numel()), st) == 4
    # the workspace holds doubles: one that is not 8-byte aligned is refused too
    ws4 = torch.empty(ws.numel() + 8, dtype=torch.uint8, device="cuda")[4:]
    assert ws4.data_ptr() % 8 == 4 and L.nvfi_ray_distortion(*args[:9], _lib.ptr(ws4), C.c_int64(ws4.numel()), st) == 4
    assert b"aligned" in L.nvfi_last_error()
    # no sample per ray, a negative ray count: error 2 (there is no upper cap on S: the kernel strides any ray in chunks of 64)
    assert L.nvfi_ray_distortion(C.c_int64(R), C.c_int(0), *args[2:], C.c_int64(ws.numel()), st) == 2
    assert L.nvfi_ray_distortion(C.c_int64(-1), *args[1:], C.c_int64(ws.numel()), st) == 2
    assert L.nvfi_ray_distortion(C.c_int64(R), C.c_int(S), None, *args[3:], C.c_int64(ws.numel()), st) == 2
    torch.cuda.synchronize()
    assert float(loss) == SENT and bool((g == SENT).all())               # nothing was launched
    assert L.nvfi_ray_distortion(*args, C.c_int64(ws.numel()), st) == 0
    torch.cuda.synchronize()
    assert float(loss) != SENT and not bool((g == SENT).any())
    # without `loss` nothing reads the workspace: none is asked for, and the gradient has the same bits
    g2 = torch.full((R, S), SENT, device="cuda")
    assert L.nvfi_ray_distortion(*args[:6], None, None, _lib.ptr(g2), None, C.c_int64(0), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(g2, g)
    # the wrappers: non-contiguous / non-fp32 input is made contiguous fp32, a CPU tensor is refused
    wd = _cu(r64.named_case("fog", R, 2 * S, 1)).double()[:, ::2]
    a = distortion_loss_raw(wd, 0.1)
    b = distortion_loss_raw(wd.float().contiguous(), 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(_lib.NvfiError):
        distortion_loss_raw(torch.rand(4, 8), 0.1)


# ---------------------------------------------------------------------------------------------------------------- field A: autograd and fused driver
def torch_distortion(w, delta):
    """the same loss in fp32 torch ops (cumsum form): what a fork of the training loop would write on out[3]"""
    winc = w.cumsum(1)
    A = winc.cumsum(1) - winc
    return (delta * (2.0 * (w * A).sum(1) + (w * w).sum(1) / 3.0)).mean()


LAM = 0.5
_FA = {}


def field_a():
    if not _FA:
        gold = np.load(os.path.join(GOLD, "hotpath.npz"))
        model, meta = make_model("A")
        f = model.nvfi
        _FA.update(model=model, f=f, o=_cu(gold["A:rays_o"]), d=_cu(gold["A:rays_d"]), u=torch.from_numpy(gold["A:train_nonkey:u"].copy()),
                   tgt=_cu(gold["A:train_nonkey:target"]), t=0.38 * f.tmax / (f.num_keyframes - 1))
    return _FA


def _autograd(c, dist_fn, lam, depth_gt=None, depth_w=0.0):
    from nvfi_amd.utils import compute_depth_loss
    model, f = c["model"], c["f"]
    model.zero_grad(set_to_none=True)
    f.train()
    f.jitter_override = c["u"]
    try:
        out = f(c["t"], c["o"], c["d"], True)
    finally:
        f.jitter_override = None
    mse = torch.nn.functional.mse_loss(out[0], c["tgt"])
    total = mse
    dist = dl = None
    if lam:
        dist = dist_fn(out[3], f.distortion_delta())
        total = total + lam * dist
    if depth_gt is not None:
        dl = compute_depth_loss(out[1], depth_gt)
        total = total + depth_w * dl
    total.backward()
    return dict(mse=float(mse.detach()), dist=None if dist is None else dist.detach().clone(), dl=None if dl is None else dl.detach().clone(),
                rgb=out[0].detach().clone(), weights=out[3].detach().clone(), g=named_grads(model))


def _same_grads(g, ref, label):
    n = 0
    for k, r in ref.items():
        if r is None:
            continue
        e = relerr(g[k], r)
        assert e < 2e-5, (label, k, e)
        n += 1
    assert n >= 19


def test_autograd_wrapper_matches_torch_ops_on_field_a():
    from nvfi_amd.utils import distortion_loss
    c = field_a()
    ref = _autograd(c, torch_distortion, LAM)
    got = _autograd(c, distortion_loss, LAM)
    assert torch.equal(got["rgb"], ref["rgb"]) and torch.equal(got["weights"], ref["weights"])
    y = r64.index_form(ref["weights"].cpu().numpy(), c["f"].distortion_delta())
    e_k, e_t = abs(float(got["dist"]) - y["loss"]) / y["loss"], abs(float(ref["dist"]) - y["loss"]) / y["loss"]
    print(f"distortion of field A's weights: {y['loss']:.6e}; kernel err {e_k:.2e}, torch-op err {e_t:.2e}")
    assert e_k <= bounds()["loss"] and got["dist"].dim() == 0
    _same_grads(got["g"], ref["g"], "autograd wrapper")
    # the term reaches the parameters: lambda is large enough that the density-plane gradients differ by more than 10 x the tolerance
    none = _autograd(c, None, 0.0)
    moved = maxrel(none["g"]["density_plane_space.0"], ref["g"]["density_plane_space.0"])
    print("density_plane_space.0 with / without the term:", moved)
    assert moved > 10 * 2e-5
    # the field's own method and NVFi's are the same call
    w = ref["weights"]
    assert torch.equal(c["f"].distortion_loss(w), distortion_loss(w, c["f"].distortion_delta()))
    assert torch.equal(c["model"].distortion_loss(w), c["f"].distortion_loss(w))
    c["model"].zero_grad(set_to_none=True)


def test_fused_driver_matches_the_autograd_route():
    c = field_a()
    model, f = c["model"], c["f"]
    uj = c["u"].cuda().reshape(-1)
    ref = _autograd(c, torch_distortion, LAM)

    def fused(**kw):
        model.zero_grad(set_to_none=True)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        f.train()
        return f.render_mse_backward_(c["t"], c["o"], c["d"], c["tgt"], white_bg=True, jitter=uj, **kw)

    res = fused(distortion_weight=LAM)
    assert len(res) == 3
    loss, rgb, dist = res
    assert torch.equal(rgb, ref["rgb"])
    assert abs(float(loss) - ref["mse"]) <= 2e-6 * abs(ref["mse"])
    y = r64.index_form(ref["weights"].cpu().numpy(), f.distortion_delta())
    assert dist.dim() == 0 and abs(float(dist) - y["loss"]) <= bounds()["loss"] * y["loss"]
    assert abs(float(dist) - float(ref["dist"])) <= 2e-6 * abs(float(ref["dist"]))
    _same_grads(named_grads(model), ref["g"], "fused")
    dist_bits = dist.cpu().numpy().tobytes()
    # without the term: the two-tuple, the same bits with and without the argument, and other gradients
    r0 = fused()
    g0 = named_grads(model)
    r00 = fused(distortion_weight=0.0)
    assert len(r0) == 2 and len(r00) == 2
    assert r0[0].cpu().numpy().tobytes() == r00[0].cpu().numpy().tobytes() and torch.equal(r0[1], r00[1])
    # ... and the same gradients: the two calls make the same launches with the same arguments.  Compared at the tolerance, not bit for bit: the
    # plane-gradient scatter's default path adds in an order that differs from run to run (tests/test_gpu_edges.py::test_deterministic_mode)
    g00 = named_grads(model)
    assert set(g00) == set(g0)
    _same_grads(g00, g0, "distortion_weight=0.0")
    moved = maxrel(g0["density_plane_space.0"], ref["g"]["density_plane_space.0"])
    assert moved > 10 * 2e-5, moved
    # loss_scale scales the distortion gradient too, not the value
    r4 = fused(distortion_weight=LAM, loss_scale=0.25)
    assert r4[2].cpu().numpy().tobytes() == dist_bits
    assert relerr(named_grads(model)["density_plane_space.0"], 0.25 * ref["g"]["density_plane_space.0"]) < 2e-5
    # with the depth term on: (loss, rgb, depth_loss, distortion), every gradient of the three-term loss
    R = c["o"].shape[0]
    gt = _cu(np.random.default_rng(3).uniform(float(f.near_far[0]), float(f.near_far[1]), R).astype(np.float32))
    ref3 = _autograd(c, torch_distortion, LAM, depth_gt=gt, depth_w=0.3)
    res = fused(target_depth=gt, depth_weight=0.3, distortion_weight=LAM)
    assert len(res) == 4
    assert abs(float(res[2]) - float(ref3["dl"])) <= 2e-6 * abs(float(ref3["dl"]))
    assert res[3].cpu().numpy().tobytes() == dist_bits
    _same_grads(named_grads(model), ref3["g"], "fused + depth")
    with pytest.raises(ValueError):
        fused(distortion_weight=-1.0)
    model.zero_grad(set_to_none=True)


def test_evaluation_reports_the_floater_map():
    from nvfi_amd.models import Camera, Renderer
    from nvfi_amd.utils import distortion_loss_raw, render_test_evaluation
    c = field_a()
    model, f = c["model"], c["f"]
    H = W = 32
    near, far = [float(v) for v in f.near_far]
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, 4.0])
    ren = Renderer(model, 0, 0, 2048)
    res = render_test_evaluation(model, ren, [pose.numpy()] * 2, [0.0, c["t"]], None, H, W, 40.0, near, far, update_alpha_mask=False, with_distortion=True)
    assert res["distortion_maps"].shape == (2, H, W) and res["distortion_maps"].dtype == np.float32
    assert len(res["distortion"]) == 2 and res["mean_distortion"] == sum(res["distortion"]) / 2
    with torch.no_grad():
        cam = Camera(pose.cuda(), H, W, 40.0, None, near, far)
        weights = ren.render(c["t"], cam.rays.to("cuda"), white_background=True, mode="test")[3]
    loss, _, per_ray = distortion_loss_raw(weights.reshape(H * W, -1), model.distortion_delta(), want_per_ray=True)
    assert res["distortion_maps"][1].tobytes() == per_ray.cpu().numpy().tobytes()
    assert res["distortion_maps"][1].max() > 0.0
    mean = float(per_ray.cpu().numpy().astype(np.float64).mean())
    assert abs(res["distortion"][1] - mean) <= bounds()["loss"] * mean and res["distortion"][1] == float(loss)
    plain = render_test_evaluation(model, ren, [pose.numpy()], [0.0], None, H, W, 40.0, near, far, update_alpha_mask=False)
    assert "distortion" not in plain and "distortion_maps" not in plain
    f.train()
