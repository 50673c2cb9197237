"""The rest of a training iteration on the GPU - the plane regularisers (nvfi_plane_regs / _dev behind regularizers_backward_ and the three
reference-signature methods, csrc/regs.hip), the one-launch Adam (nvfi_amd.optim.Adam, csrc/optim.hip) and the one-launch MSE (k_mse) -
against the float64 yardstick tests/optim64.py, which tests/test_optim64_golden.py pins to the reference's goldens and to torch in float64.

Bounds.  No tolerance is typed in.  For every case and quantity the bound is computed here, on the CPU, from the yardstick alone and printed next to
the device's error:  bound = 4 x max(maxrel, rel_l2) of the yardstick evaluated in float32 against itself in float64 on that same case (the
relative error for a scalar), and never less than 4 fp32 spacings of the quantity's peak (optim64.bound).  The floor is what decides where the
float32 evaluation is exact or correctly rounded: a result stored in fp32 is up to half a spacing away from the float64 value however it was
computed, so a single number (a loss value, a one-element tensor) cannot be held to a multiple of another single number's rounding luck.
Gradient passes run into a .grad that already holds noise; what is compared is what was ADDED (after - before, formed in float64), and the
yardstick's float32 evaluation includes that one fp32 addition.  The noise is scaled per plane to the peak of the yardstick's gradient, so the
addition does not swamp the gradient.  A plane that must receive nothing has to keep its noise bit for bit.
Nothing here has a near-tie band (the L1 sign is taken on the fp32 plane value itself): no element is exempt.

Measured (MI355X; worst over the cases of a group; "fp32" = the yardstick's float32 evaluation, "device" = the HIP kernels, both against float64):
    quantity (cases)                                        fp32 evaluation        device                 bound
    regs values, (7, 5, 9)                                  3.0e-08 .. 4.4e-08     3.0e-08 .. 4.4e-08     2.9e-07 .. 4.1e-07 (the floor)
    regs values, (37, 50, 41)                               2.2e-09 .. 2.1e-08     2.2e-09 .. 2.1e-08     2.6e-07 .. 3.7e-07 (the floor)
    regs values, (130, 97, 61)                              1.5e-08 .. 8.4e-08     4.3e-09 .. 4.1e-08     2.5e-07 .. 3.5e-07 (the floor)
    regs added gradients, plane closest to its bound        1.6e-07 .. 2.5e-07     2.0e-07 .. 2.9e-07     6.4e-07 .. 1.0e-06
    adam p / exp_avg / exp_avg_sq, all cases                3.4e-08 .. 1.7e-07     equal to the fp32 evaluation in every tensor        1.0 x 4
    adam exp_avg_sq at |g| ~ 1e-20 (subnormal g^2)          6.8e-06                6.8e-06                2.7e-05
    mse value                                               1.7e-08 .. 9.1e-08     1.7e-09 .. 6.0e-08     3.1e-07 .. 4.1e-07 (the floor)
    mse gradient (x upstream factor)                        0 .. 1.0e-07           0 .. 1.3e-07           3.2e-07 .. 4.0e-07
The regulariser values are the same in every call and every gradient mode.  They were not when these tests were written: the workgroups of
k_plane_regs added fp32 partials to the three output floats, 288 to 576 atomics per value in arrival order, and on the (130, 97, 61) grid L1 came
out at 3.6e-07 .. 4.5e-07 against 3.5e-07, TVd at 2.6e-07 against 2.5e-07 and TVa at 3.5e-07 .. 5.1e-07 against 3.1e-07, different from call to
call.  The partials are now summed in double and rounded to fp32 once (regs.hip).  The stale-value case failed before optim.GENERATION entered the
key of _RegFn.forward: the values moved by 0 where the yardstick moved by 4.2e-02 (L1), 1.8e-01 (TVd) and 4.5e-01 (TVa).

Sensitivity.  Mutations of the yardstick must move the compared quantity by more than 3 x its bound (asserted below): a plane without the
vertical difference into its last row, time planes without the factor 3, a plane without the last four channels of its last texel; tensor 48
with the learning rate of tensor 47 and tensor 96 with that of tensor 48; an MSE divided by n - 1.
Two work-skipping mutations of the LIBRARY were built in a scratch copy and this file run once against each (34 tests):
    k_plane_regs ignoring `y > 0`                     12 failed: all three grids of test_regularizers_backward_host_and_device_weights and all nine
                                                      cases of test_reference_signature_methods (the gradient of every plane with a TV term)
    adam_impl passing hyper_base = 0 to every launch  2 failed: test_adam_more_tensors_than_one_launch_holds[49-dev] and [97-dev] (the host path does
                                                      not read hyper_dev and passed, as it should)

Run this file as the GPU suite does: under `timeout`, with -x, so that the run ends at the first fault."""
import numpy as np
import pytest
import torch

import optim64 as o64
from helpers import make_model

pytestmark = pytest.mark.gpu
MARGIN = 4.0
W3 = (8e-4, 0.7, 1.3)
GRIDS = {"tiny": ((7, 5, 9), 2), "mid": ((37, 50, 41), 16), "big": ((130, 97, 61), 4)}
SWEEP = 96 * 1024 * 4          # floats one grid sweep of k_plane_regs covers
QV = ("L1", "TVd", "TVa")
_CASES, _YARD = {}, {}


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np(t):
    return t.detach().cpu().contiguous().numpy()


def _planes12(f):
    return list(f.density_plane_space) + list(f.density_plane_time) + list(f.app_plane_space) + list(f.app_plane_time)


def build_field(name):
    """field A re-gridded to GRIDS[name], a scattered 5 % of the space-plane entries exactly 0.0 and 5 % of the time-plane entries exactly 1.0"""
    G, K = GRIDS[name]
    model, _ = make_model("A")
    f = model.nvfi
    f.upsample_volume_grid(list(G), K)
    rng = np.random.default_rng(sum(G))
    with torch.no_grad():
        for k, p in enumerate(_planes12(f)):
            a = _np(p)
            time = k // 3 in (1, 3)
            a[rng.random(a.shape) < 0.05] = 1.0 if time else 0.0
            p.copy_(torch.from_numpy(a))
            assert p.is_contiguous(memory_format=torch.channels_last)
    return model


def case(name):
    """the field of a grid (built once), its planes as numpy, and per-plane gradient noise scaled to the yardstick's gradient peak"""
    if name not in _CASES:
        model = build_field(name)
        f = model.nvfi
        K = GRIDS[name][1]
        planes = [_np(p) for p in _planes12(f)]
        assert all((planes[k] == 0).mean() > 0.03 for k in (0, 1, 2, 6, 7, 8)) and all((planes[k] == 1).mean() > 0.03 for k in (3, 4, 5))
        _, g = o64.regs(planes[:9], K, W3)
        rng = np.random.default_rng(7)
        noise = []
        for k, p in enumerate(planes):
            peak = float(np.abs(g[k]).max()) if k < 9 else 1e-6
            n = (rng.standard_normal(p.shape) * peak).astype(np.float32)
            n[n == 0] = np.float32(peak)
            noise.append(n)
        _CASES[name] = dict(model=model, f=f, K=K, planes=planes, noise=noise)
    return _CASES[name]


def yard(name, w3):
    """yardstick of one (grid, weights): values, accumulated gradients and what was added, in float64 and float32, and the bounds"""
    key = (name, tuple(w3))
    if key not in _YARD:
        c = case(name)
        out = {}
        for tag, dt in (("64", np.float64), ("32", np.float32)):
            vals, after = o64.regs(c["planes"][:9], c["K"], w3, dtype=dt, g0=c["noise"][:9])
            out["v" + tag] = [float(v) for v in vals]
            out["a" + tag] = [a.astype(np.float64) - n for a, n in zip(after, c["noise"])]
        out["bv"] = [o64.bound(a, b, MARGIN) for a, b in zip(out["v32"], out["v64"])]
        out["ba"] = [o64.bound(a, b, MARGIN) for a, b in zip(out["a32"], out["a64"])]
        _YARD[key] = out
    return _YARD[key]


def set_noise(c):
    for p, n in zip(_planes12(c["f"]), c["noise"]):
        p.grad = torch.empty_like(p).copy_(torch.from_numpy(n).cuda())
        assert p.grad.stride() == p.stride()


def check_regs(label, name, w3, vals):
    """vals: the device's (L1, TVd, TVa), None where the call does not return one; the planes' .grad hold noise + what the call added"""
    c, y = case(name), yard(name, w3)
    bad, line = [], []
    for i, q in enumerate(QV):
        if vals[i] is None:
            continue
        e = o64.err(float(vals[i]), y["v64"][i])
        line.append(f"{q} {e:.2e}/{y['bv'][i]:.2e} (fp32 {o64.err(y['v32'][i], y['v64'][i]):.2e})")
        if not e <= y["bv"][i]:
            bad.append((q, e, y["bv"][i]))
    worst = (0.0, None)
    for k, p in enumerate(_planes12(c["f"])):
        if k >= 9 or not y["a64"][k].any():       # a plane this call must not touch
            assert _bits_equal(p.grad, torch.from_numpy(c["noise"][k]).cuda()), (label, "plane", k, "was written")
            continue
        added = _np(p.grad).astype(np.float64) - c["noise"][k]
        e, b = o64.err(added, y["a64"][k]), y["ba"][k]
        if e / b >= worst[0]:
            worst = (e / b, f"plane {k}: {e:.2e}/{b:.2e} (fp32 {o64.err(y['a32'][k], y['a64'][k]):.2e})")
        if not e <= b:
            bad.append((f"grad{k}", e, b))
    print(f"[optim64] regs {name} {label}: device/bound " + ", ".join(line) + f"; gradient closest to its bound: {worst[1]}")
    assert not bad, (label, name, bad)


# ------------------------------------------------------------------------------------------------ plane regularisers
def test_grids_enter_the_paths_they_are_meant_to():
    sizes = {n: [p.size for p in case(n)["planes"][:9]] for n in GRIDS}
    assert max(sizes["tiny"]) < 1024 * 4                                            # every plane below ONE workgroup's share
    # the largest appearance plane (48 x 97 x 130) takes two sweeps, the other two (380 640 and 284 016 floats) and every density plane take one
    assert max(sizes["big"][6:]) > SWEEP > min(sizes["big"][6:]) and max(sizes["big"][:6]) < SWEEP
    assert case("tiny")["K"] == 2 and max(sizes["mid"]) < SWEEP


@pytest.mark.parametrize("name", list(GRIDS))
def test_regularizers_backward_host_and_device_weights(name):
    c = case(name)
    f = c["f"]
    for label, w3, dev in (("host weights", W3, False), ("device weights", W3, True), ("device weights, TVd weight 0", (W3[0], 0.0, W3[2]), True),
                           ("device weights, L1 weight 0", (0.0, W3[1], W3[2]), True)):
        set_noise(c)
        out = f.regularizers_backward_(torch.tensor(w3, dtype=torch.float32, device="cuda")) if dev else f.regularizers_backward_(*w3)
        check_regs(label, name, w3, out.cpu().numpy())


@pytest.mark.parametrize("mode", [False, True, "arena"], ids=["autograd", "inplace", "arena"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_reference_signature_methods(name, mode):
    from nvfi_amd.utils import TVLoss
    c = case(name)
    f = c["f"]
    tv = TVLoss()
    f.accumulate_grads_inplace = mode
    try:
        set_noise(c)
        vals = [f.density_L1(), f.TV_loss_density(tv), f.TV_loss_app(tv)]
        (W3[0] * vals[0] + W3[1] * vals[1] + W3[2] * vals[2]).backward()
        check_regs(f"three methods in one loss ({mode})", name, W3, [v.item() for v in vals])
        set_noise(c)
        v = f.TV_loss_app(tv)
        (W3[2] * v).backward()
        check_regs(f"TV_loss_app alone ({mode})", name, (0.0, 0.0, W3[2]), [None, None, v.item()])
        set_noise(c)
        a, b = f.density_L1(), f.density_L1()
        (a + b).backward()
        assert a.item() == b.item()
        check_regs(f"2 * density_L1 from two calls ({mode})", name, (2.0, 0.0, 0.0), [a.item(), None, None])
    finally:
        f.accumulate_grads_inplace = False


def test_regs_bounds_see_a_subtly_wrong_kernel():
    """mutations of the yardstick on the (7, 5, 9) field move the compared quantity by more than 3 x its bound"""
    c, y = case("tiny"), yard("tiny", W3)
    for mut, iv, planes in (("last_row", 2, (6,)), ("no_t3", 1, (3, 4, 5)), ("last4", 0, (0,))):
        vals, after = o64.regs(c["planes"][:9], c["K"], W3, g0=c["noise"][:9], mutate=mut)
        e = o64.err(float(vals[iv]), y["v64"][iv])
        print(f"[optim64] sensitivity {mut}: {QV[iv]} moves {e:.2e} (bound {y['bv'][iv]:.2e})")
        assert e > 3 * y["bv"][iv], (mut, QV[iv], e)
        for k in planes:
            e = o64.err(after[k] - c["noise"][k], y["a64"][k])
            print(f"[optim64] sensitivity {mut}: gradient of plane {k} moves {e:.2e} (bound {y['ba'][k]:.2e})")
            assert e > 3 * y["ba"][k], (mut, k, e)


def test_values_follow_the_planes_through_an_optimiser_step():
    """The value triple is shared by the calls of ONE iteration: three forward calls without an optimiser step in between return entries of one
    launch.  nvfi_amd.optim.Adam writes the planes through raw pointers (no `_version` bump), so a triple kept from calls that never ran a
    backward (no_grad: logging) must not survive the step."""
    from nvfi_amd.models.tensorf_keyframe import _rt
    from nvfi_amd.optim import Adam
    from nvfi_amd.utils import TVLoss
    name = "mid"
    model = build_field(name)
    f, K = model.nvfi, GRIDS[name][1]
    tv = TVLoss()

    def triple():
        return [f.density_L1().item(), f.TV_loss_density(tv).item(), f.TV_loss_app(tv).item()]

    def yardstick():
        planes = [_np(p) for p in _planes12(f)[:9]]
        v64, _ = o64.regs(planes, K, W3)
        v32, _ = o64.regs(planes, K, W3, dtype=np.float32)
        return [float(v) for v in v64], [o64.bound(a, b, MARGIN) for a, b in zip(v32, v64)]

    # one pass per iteration: the library's launch profile has no class for k_plane_regs, so the shared entry itself is watched
    entries = []
    for fn in (f.density_L1, lambda: f.TV_loss_density(tv), lambda: f.TV_loss_app(tv)):
        v = fn()
        assert v.requires_grad
        entries.append((_rt(f)["_reg_fwd"], v.item()))
    assert entries[0][0] is entries[1][0] is entries[2][0]
    assert [e[1] for e in entries] == entries[0][0][1].tolist()
    with torch.no_grad():
        first = triple()
    assert _rt(f)["_reg_fwd"] is entries[0][0] and first == [e[1] for e in entries]
    y0, b0 = yardstick()
    model.zero_grad(set_to_none=True)
    f.regularizers_backward_(*W3)
    opt = Adam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    opt.step()
    y1, b1 = yardstick()
    with torch.no_grad():
        second = triple()
    bad = []
    for i, q in enumerate(QV):
        b = max(b0[i], b1[i])
        move = o64.err(y1[i], y0[i])
        assert move > 10 * b, (q, "the yardstick itself did not move", move)
        e0, e1, d = o64.err(first[i], y0[i]), o64.err(second[i], y1[i]), o64.err(second[i], first[i])
        print(f"[optim64] stale values: {q}: before the step {e0:.2e}, after it {e1:.2e} (bound {b:.2e}); the value moved by {d:.2e}, the yardstick by {move:.2e}")
        if not (e0 <= b0[i] and e1 <= b1[i] and d > 10 * b):
            bad.append((q, e0, e1, d, b))
    assert not bad, bad
    assert _rt(f)["_reg_fwd"] is not entries[0][0]


# ------------------------------------------------------------------------------------------------ Adam
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4100)
B1, B2, EPS = 0.9, 0.99, 1e-8


def _lr(k):
    return 1e-4 * 2.0 ** (k % 7)          # neighbours differ by x2 (x64 at the wrap); tensor k and tensor k - 48 never share one


def _params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in sizes]


def _grads(sizes, steps, seed, none_before=None):
    rng = np.random.default_rng(seed)
    return [[None if (none_before and s < none_before.get(k, 0)) else (rng.standard_normal(n) * 10.0 ** (s % 3 - 1)).astype(np.float32)
             for s in range(steps)] for k, n in enumerate(sizes)]


def drive(ps, lrs, gs, path="host", opt=None):
    """5 (len(gs[0])) steps of nvfi_amd.optim.Adam, one group per tensor, zero_grad alternating, every lr rescaled after every step.
    path "dev": the first step on the host path, the others through next_hyper() + step(hyper_dev=...).  -> optimiser, the lr every tensor saw"""
    from nvfi_amd.optim import Adam
    if opt is None:
        opt = Adam([dict(params=[p], lr=lr) for p, lr in zip(ps, lrs)], betas=(B1, B2), eps=EPS)
    seen = [[] for _ in ps]
    for s in range(len(gs[0])):
        for k, p in enumerate(ps):
            if gs[k][s] is None:
                p.grad = None
                continue
            t = torch.from_numpy(gs[k][s]).cuda().reshape(p.shape)
            if p.grad is None:
                p.grad = t.clone()
            else:
                p.grad.copy_(t)         # same buffer: the optimiser's pointer table is reused
            seen[k].append(opt.param_groups[k]["lr"])
        zg = s % 2 == 0
        before = [None if p.grad is None else p.grad.clone() for p in ps]
        if path == "dev" and s > 0:
            h = opt.next_hyper()
            assert len(h) == 1 + sum(p.grad is not None for p in ps)
            opt.step(zero_grad=zg, hyper_dev=torch.tensor(h, dtype=torch.float32, device="cuda"))
        else:
            opt.step(zero_grad=zg)
        for k, (p, b) in enumerate(zip(ps, before)):
            if b is not None:
                assert _bits_equal(p.grad, torch.zeros_like(b) if zg else b), (k, s, "gradient after the step")
        for grp in opt.param_groups:
            grp["lr"] *= 0.83
    return opt, seen


def check_adam(label, ps, p0, gs, seen, opt, state0=None, t0=0):
    """every tensor's p, exp_avg, exp_avg_sq against the yardstick under its own bound -> {(k, quantity): (yardstick64, bound)}"""
    ref, bad = {}, []
    worst = {q: (-1.0, "") for q in ("p", "exp_avg", "exp_avg_sq")}
    for k, p in enumerate(ps):
        if p.numel() == 0:
            continue
        g_seq = [g for g in gs[k] if g is not None]
        m0, v0 = state0[k] if state0 else (None, None)
        y64 = o64.adam(p0[k], g_seq, seen[k], B1, B2, EPS, m0, v0, t0)
        y32 = o64.adam(p0[k], g_seq, seen[k], B1, B2, EPS, m0, v0, t0, dtype=np.float32)
        st = opt.state[p]
        assert int(st["step"]) == t0 + len(g_seq), (label, k, st["step"])
        for q, dev, a64, a32 in zip(("p", "exp_avg", "exp_avg_sq"), (p, st["exp_avg"], st["exp_avg_sq"]), y64, y32):
            b, e = o64.bound(a32, a64, MARGIN), o64.err(_np(dev).reshape(-1), a64)
            ref[(k, q)] = (a64, b)
            r = e / b if b > 0 else (0.0 if e == 0 else np.inf)
            if r > worst[q][0]:
                worst[q] = (r, f"tensor {k} (n={p.numel()}): {e:.2e}/{b:.2e} (fp32 {o64.err(a32, a64):.2e})")
            if not e <= b:
                bad.append((k, q, e, b))
    print(f"[optim64] adam {label}: closest to its bound, device/bound: " + "; ".join(f"{q} {w[1]}" for q, w in worst.items()))
    assert not bad, (label, bad[:8])
    return ref


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("T", [49, 97])
def test_adam_more_tensors_than_one_launch_holds(T, path):
    """49 / 97 tensors: two / three launches, the later ones index hyper_dev from hyper_base"""
    sizes = [SIZES[k % len(SIZES)] for k in range(T)]
    lrs = [_lr(k) for k in range(T)]
    ps = _params(sizes, T)
    p0 = [_np(p) for p in ps]
    gs = _grads(sizes, 5, T + 1)
    opt, seen = drive(ps, lrs, gs, path)
    ref = check_adam(f"{T} tensors, {path} path", ps, p0, gs, seen, opt)
    # the bound sees a tensor that was updated with another tensor's learning rate
    for k, other in ((48, 47),) if T == 49 else ((96, 48),):
        assert all(abs(a / b - 1) >= 1 - 1e-9 or abs(b / a - 1) >= 1 - 1e-9 for a, b in zip(seen[k], seen[other]))
        mut = o64.adam(p0[k], gs[k], seen[other], B1, B2, EPS)[0]
        a64, b = ref[(k, "p")]
        e = o64.err(mut, a64)
        print(f"[optim64] sensitivity: tensor {k} with the lr of tensor {other}: p moves {e:.2e} (bound {b:.2e})")
        assert e > 3 * b


def test_adam_vector_and_scalar_paths_and_two_stride_sweeps_in_one_launch():
    """a 3-element tensor, a tensor above 2048 x 256 x 4 elements (capped grid: the stride loop runs twice) and a parameter that starts one float
    into a larger buffer (n % 4 == 0: only its alignment sends it to the scalar path), whose neighbours must not be written"""
    n_big, n_view = 2048 * 256 * 4 + 4100, 1024
    g = torch.Generator().manual_seed(11)
    buf = torch.randn(n_view + 8, generator=g).cuda()
    ps = _params([3, n_big], 12) + [torch.nn.Parameter(buf[1:1 + n_view])]
    assert ps[2].data_ptr() == buf.data_ptr() + 4 and ps[2].data_ptr() % 16 and ps[1].data_ptr() % 16 == 0
    keep = buf.clone()
    sizes = [3, n_big, n_view]
    p0 = [_np(p) for p in ps]
    gs = _grads(sizes, 5, 13)
    opt, seen = drive(ps, [_lr(k) for k in range(3)], gs)
    check_adam("3 + 2 101 252 + misaligned 1024", ps, p0, gs, seen, opt)
    assert _bits_equal(buf[:1], keep[:1]) and _bits_equal(buf[1 + n_view:], keep[1 + n_view:])
    assert not _bits_equal(buf[1:1 + n_view], keep[1:1 + n_view])


def test_adam_exact_zero_gradients_on_fresh_state():
    from nvfi_amd.optim import Adam
    sizes = [1024, 1025]
    ps = _params(sizes, 21)
    p0 = [p.detach().clone() for p in ps]
    rng = np.random.default_rng(22)
    gs = []
    for p, n in zip(ps, sizes):
        g = rng.standard_normal(n).astype(np.float32)
        g[rng.random(n) < 0.3] = 0.0
        gs.append([g])
        p.grad = torch.from_numpy(g).cuda()
    opt = Adam([dict(params=[p], lr=_lr(k)) for k, p in enumerate(ps)], betas=(B1, B2), eps=EPS)
    opt.step()
    for k, p in enumerate(ps):
        z = torch.from_numpy(gs[k][0] == 0).cuda()
        assert z.sum() > 200
        assert _bits_equal(p.detach()[z], p0[k][z]) and not opt.state[p]["exp_avg"][z].any() and not opt.state[p]["exp_avg_sq"][z].any()
        assert (p.detach()[~z] != p0[k][~z]).all()
    check_adam("exact zeros in the gradient", ps, [_np(p) for p in p0], gs, [[_lr(0)], [_lr(1)]], opt)


def test_adam_tiny_and_huge_gradients():
    sizes = [1024, 1025, 1024, 1025]
    ps = _params(sizes, 31)
    p0 = [_np(p) for p in ps]
    gs = _grads(sizes, 5, 32)
    for k, scale in enumerate((1e-20, 1e-20, 1e10, 1e10)):
        gs[k] = [(g * np.float32(scale)).astype(np.float32) for g in gs[k]]
    opt, seen = drive(ps, [_lr(k) for k in range(4)], gs)
    check_adam("|g| ~ 1e-20 and 1e+10", ps, p0, gs, seen, opt)


def test_adam_two_step_counts_share_one_table_key():
    """a parameter without a gradient in the first two steps: two batches (step counts 3 and 1) under one (betas, eps) cache key.  step(hyper_dev=)
    serves one step count only: it raises and changes nothing"""
    from nvfi_amd._lib import NvfiError
    sizes = [1024, 65, 4100]
    ps = _params(sizes, 41)
    p0 = [_np(p) for p in ps]
    gs = _grads(sizes, 5, 42, none_before={2: 2})
    opt, seen = drive(ps, [_lr(k) for k in range(3)], gs)
    assert [opt.state[p]["step"] for p in ps] == [5, 5, 3] and len(seen[2]) == 3
    check_adam("two step counts", ps, p0, gs, seen, opt)
    for p in ps:
        p.grad.normal_()
    keep = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    with pytest.raises(NvfiError):
        opt.next_hyper()
    assert [opt.state[p]["step"] for p in ps] == [5, 5, 3]           # a refused next_hyper() leaves the counters alone
    with pytest.raises(NvfiError):
        opt.step(hyper_dev=torch.ones(4, device="cuda"))
    torch.cuda.synchronize()
    for p, (a, m, v) in zip(ps, keep):
        assert _bits_equal(p.detach(), a) and _bits_equal(opt.state[p]["exp_avg"], m) and _bits_equal(opt.state[p]["exp_avg_sq"], v)


def test_adam_continues_a_loaded_state_at_step_30000():
    from nvfi_amd.optim import Adam
    sizes = [1024, 65]
    ps = _params(sizes, 51)
    p0 = [_np(p) for p in ps]
    rng = np.random.default_rng(52)
    state0 = [((0.1 * rng.standard_normal(n)).astype(np.float32), (0.01 * rng.random(n) + 1e-6).astype(np.float32)) for n in sizes]
    opt = Adam([dict(params=[p], lr=_lr(k)) for k, p in enumerate(ps)], betas=(B1, B2), eps=EPS)
    sd = opt.state_dict()
    sd["state"] = {k: {"step": torch.tensor(30000.0), "exp_avg": torch.from_numpy(m), "exp_avg_sq": torch.from_numpy(v)} for k, (m, v) in enumerate(state0)}
    opt.load_state_dict(sd)         # the layout of a torch.optim.Adam checkpoint: a tensor step count, CPU moments
    gs = _grads(sizes, 5, 53)
    opt, seen = drive(ps, None, gs, opt=opt)
    check_adam("state loaded at step 30000", ps, p0, gs, seen, opt, state0=state0, t0=30000)


def test_adam_empty_parameter_between_two_others():
    from nvfi_amd._lib import NvfiError
    sizes = [65, 0, 1024]
    ps = _params(sizes, 61)
    p0 = [_np(p) for p in ps]
    gs = _grads(sizes, 5, 62)
    lrs = [_lr(0), _lr(3), _lr(1)]
    opt, seen = drive(ps, lrs, gs)          # host path: the neighbours are updated, each with its own lr
    check_adam("an empty tensor in the table", ps, p0, gs, seen, opt)
    for p in ps:
        p.grad.normal_()
    keep = [p.detach().clone() for p in ps]
    h = opt.next_hyper()
    assert len(h) == 4
    with pytest.raises(NvfiError):          # hyper_dev is indexed by table position: an empty tensor is refused before anything is launched
        opt.step(hyper_dev=torch.tensor(h, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert all(_bits_equal(p.detach(), a) for p, a in zip(ps, keep))


# ------------------------------------------------------------------------------------------------ MSE
def check_mse(label, x, y, factor=3.0):
    from nvfi_amd.utils import mse_loss
    xn, yn = _np(x), _np(y)
    x = x.detach().requires_grad_()
    (factor * mse_loss(x, y)).backward()
    val = mse_loss(x.detach(), y).item()
    v64, g64 = o64.mse(xn, yn)
    v32, g32 = o64.mse(xn, yn, dtype=np.float32)
    g64, g32 = factor * g64, np.float32(factor) * g32
    bv, bg = o64.bound(v32, v64, MARGIN), o64.bound(g32, g64, MARGIN)
    ev, eg = o64.err(val, v64), o64.err(_np(x.grad), g64)
    print(f"[optim64] mse {label}: value {ev:.2e}/{bv:.2e} (fp32 {o64.err(v32, v64):.2e}), gradient {eg:.2e}/{bg:.2e} (fp32 {o64.err(g32, g64):.2e})")
    assert x.grad.shape == x.shape and ev <= bv and eg <= bg, (label, ev, bv, eg, bg)
    if xn.size > 1:
        vm, gm = o64.mse(xn, yn, mutate="n-1")
        assert o64.err(vm, v64) > 3 * bv and o64.err(factor * gm, g64) > 3 * bg, (label, "the bound does not see a division by n - 1")


@pytest.mark.parametrize("n", [1, 63, 65, 1023, 1025, 6144, 65536, 65537])
def test_mse_value_and_gradient(n):
    """one value, ragged sizes around the wave and the workgroup, the shipped batch, the largest size the kernel takes, and 65 537 (torch)"""
    g = torch.Generator(device="cuda").manual_seed(n)
    check_mse(f"n={n}", torch.rand(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g))


def test_mse_non_contiguous_input():
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(2048, 3, device="cuda", generator=g).t()
    assert not x.is_contiguous()
    check_mse("transposed (3, 2048)", x, torch.rand(3, 2048, device="cuda", generator=g), factor=0.37)
