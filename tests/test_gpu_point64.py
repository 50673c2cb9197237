"""The stand-alone point queries on the device - nvfi_vel_eval, nvfi_integrate_pos (csrc/abi.hip), nvfi_density_at, nvfi_app_at, nvfi_render_mlp,
nvfi_sh_render (csrc/render_blocks.hip) and their Python wrappers - against their float64 restatement tests/point64.py, which
tests/test_point64_golden.py pins to the reference's goldens.  The float64 references run in torch on the GPU.

Fields: A (VelocityAABB, K = 4), B (VelocityAABBSur, K = 16: step rejection), D (A's geometry with SH shading).  Sizes: alpha64.SIZES - the 32-point
wave tile, the 128-point workgroup, the 256-thread pack / unpack blocks, the 32-point blocks of k_density_q, one point over 2^15.
Bound of every comparison, per element: |got - ref| <= rtol |ref| + atol with point64.POINT_RTOL / POINT_ATOL of the (call, field, case): exactly 3 x
the float32 evaluation of the yardstick against its float64 evaluation on the same cases (never under one fp32 ulp), measured on the CPU; none is
taken from the device.

(a) test_vel_eval: xt over 1.05 x the gate box, nine points ON the box, t in [0, 1]; un-gated all six columns; gated the zero pattern (identical to the
    yardstick's off the near-face points - and on the nine placed ones, whose decision compares equal numbers), columns 3-5 of the (N, 6) buffer
    untouched, the wrapper's (N, 3).
(b) test_integrate_pos: both integrators (x6, and vel_fp16 = "fp32": the fp32 MFMA kernels), the time cases of point64.time_cases: `none` (output =
    input bit for bit), `mixed` (0 ... several steps and both signs in a tile; t > tmax extrapolates; field B rejects steps.  Both signs, a time
    beyond tmax and n_rejected > 0 are asserted from N = 257 on: a case of 1 ... 256 random points need not hold a point that leaves the surround box),
    `one_live` (all but the last point and one per workgroup stand still, bit for bit), `forward` (t = 0 towards [0.5, 0.75): 4 - 6 steps on A,
    20 - 30 on B; N <= 257), `tiny` (one step of ~1e-8 ... 1e-6).  Near-face points are printed, finite and inside 1.2 x the box.  The wrapper leaves
    its arguments untouched and gives the same bits for (N, 1) times, float64 inputs and a non-contiguous view.
(c) test_integrate_pos_across_the_kernel_switch: x6, `mixed`, N = 32 * 4096 (the last size of k_rk2_x6<1>) and + 1 (the first of k_rk2_x6w: one live
    lane in the last tile): both against the yardstick, their common 32 * 4096 outputs bit-identical.  The threshold is NVFI_X6W_MIN_TILES = 4096
    under NVFI_X6W = 1 (csrc/switches.h): with another value in the environment the two calls could share a kernel, and the test skips.
(d) test_density_at: xyzt over 1.15 x the box, the eight special time rows at the head, up to sixteen far points at the tail (|coordinate| to 1e6,
    t' to +-50): feat is +0.0 there bit for bit, the fp32 rounding of the yardstick's exact 0 (k_density_q adds its products to a sum that starts at
    +0.0, and +0 + -0 = +0), sigma = softplus(shift).
(e) test_app_at_and_render_mlp: MLP_PE on A and B, SH on D; views randn un-normalised, features 0.3 randn; MLP_PE colours inside [0, 1];
    nvfi_sh_render against sh64 and against nvfi_render_mlp of the SH field.
(f) test_prefix_invariance: the first n outputs of a call at N = 32769 are bit-identical to the call at n on the first n inputs, n in SIZES.
(g) test_yardstick_sees_a_subtly_wrong_kernel: the device against each wrong variant of point64 falls outside the bound.
(h) in (a), (b), (e): the workspace is exactly the published size with a 4 KiB tail of 0xA5 that stays untouched; with 256 bytes less the call returns
    4 and neither the output nor any workspace byte changes.  By reading, every call tests the size before its first launch; nvfi_vel_eval,
    nvfi_integrate_pos and nvfi_render_mlp used to accept less than they publish (their plans are smaller than the published figure): they now
    refuse anything under it, like nvfi_compute_alpha.
test_use_vel_0_is_refused: the descriptor of field A (valid weight pointers) with use_vel set to 0 is refused (2) with the outputs untouched, and
    the wrappers of a use_vel=False model raise NvfiError before they touch the library.

Figures: bound (3 x the floor, or one fp32 ulp 1.19e-7) [float32 evaluation of the yardstick, CPU] / device, abs ; rel as alpha64.floors gives them,
worst over the sizes; x6 | fp32 MFMA where two device figures are shown.
  call, field, case          atol [float32] / device ; rtol [float32] / device
  vel         A              1.29e-6 [4.3e-7] / 4.5e-7 ; 5.4e-5 [1.8e-5] / 2.6e-5
  vel         B              1.11e-6 [3.7e-7] / 3.7e-7 ; 3.3e-5 [1.1e-5] / 1.3e-5
  vel gated   A              1.20e-6 [4.0e-7] / 4.5e-7 ; 7.5e-5 [2.5e-5] / 3.2e-5
  vel gated   B              1.11e-6 [3.7e-7] / 3.1e-7 ; 3.3e-5 [1.1e-5] / 1.9e-5
  integrate   A none         output == input bit for bit, both integrators, every size (B alike)
  integrate   A mixed        2.16e-7 [7.2e-8] / 1.9e-8 | 7.0e-8 ; 7.8e-6 [2.6e-6] / 3.3e-7 | 1.4e-6      (includes N = 32 * 4096 and + 1 on x6)
  integrate   A one_live     1.77e-7 [5.9e-8] / 3.6e-8 | 8.6e-8 ; 1.32e-5 [4.4e-6] / 6.5e-7 | 2.1e-6     still points: 0 bit differences
  integrate   A forward      6.3e-7 [2.1e-7] / 3.7e-8 | 1.7e-7 ; 1.92e-5 [6.4e-6] / 2.4e-6 | 5.9e-6
  integrate   A tiny         1.19e-7 [4.7e-10] / 4.6e-10 ; 1.77e-7 [5.9e-8] / 5.9e-8
  integrate   B mixed        1.19e-7 [3.6e-8] / 2.6e-8 | 3.6e-8 ; 1.83e-6 [6.1e-7] / 3.4e-7 | 6.8e-7     13 rejected steps at N = 257, 1 082 at 32769
  integrate   B one_live     1.19e-7 [1.3e-8] / 3.9e-9 | 1.2e-8 ; 1.83e-6 [6.1e-7] / 3.4e-7 | 5.5e-7
  integrate   B forward      2.55e-7 [8.5e-8] / 7.8e-8 | 8.7e-8 ; 1.71e-5 [5.7e-6] / 5.2e-6 | 5.5e-6
  integrate   B tiny         1.19e-7 [4.7e-10] / 4.6e-10 ; 1.77e-7 [5.9e-8] / 5.9e-8
  density feat  A | B        6.3e-7 [2.1e-7] / 2.0e-7 ; 3.3e-5 [1.1e-5] / 1.1e-5  |  6.6e-7 [2.2e-7] / 2.1e-7 ; 2.55e-5 [8.5e-6] / 8.6e-6
  density sigma A | B        9.9e-8 [3.3e-8] / 3.2e-8 ; 1.62e-5 [5.4e-6] / 6.1e-6  |  8.1e-8 [2.7e-8] / 2.6e-8 ; 2.28e-5 [7.6e-6] / 7.5e-6
  app_at      A | B          1.19e-7 [0] / 0 ; 4.5e-7 [1.5e-7] / 2.1e-7  |  1.19e-7 [0] / 0 ; 4.2e-7 [1.4e-7] / 2.1e-7    (no colour of these cases is under 1e-2)
  render_mlp  A, B           1.19e-7 [0] / 0 ; 4.2e-7 [1.4e-7] / 2.0e-7
  app_at      D (SH)         6.3e-6 [2.1e-6] / 2.0e-6 ; 1.44e-4 [4.8e-5] / 3.9e-5
  render_mlp  D (SH)         6.6e-7 [2.2e-7] / 2.6e-7 ; 1.98e-5 [6.6e-6] / 2.7e-6
  sh_render   D inputs       6.6e-7 [2.2e-7] / 2.0e-7 ; 1.98e-5 [6.6e-6] / 2.6e-6
  (c) 0 of 131 072 points differ between k_rk2_x6<1> and k_rk2_x6w on A and on B; (f) 0 bit differences in 19 calls x 10 sizes (8 + 8 + 3 on A, B, D).
  (g) the device leaves the bound of a wrong variant by: vel 0.8; density 1.5 - 4.8 (feat), 2e-2 - 7e-2 (sigma); app / mlp 1e-2 (A, B), 0.5 / 1.7 (D);
      sh 1.7; integrate 1.2e-4 - 4.1e-4 on A, 1.9e-5 - 7.9e-5 on B (mixed, forward, one_live; x6 and fp32 MFMA alike).
The change this comparison forced is in how the FLOOR is measured, not in the float64 yardstick and not in a kernel (tests/point64.py: FLOOR).  Against
the float32 floor of torch's blocked sums alone, the kernels that accumulate on the fp32 matrix pipe left 3 x the floor: nvfi_vel_eval on field A at
N = 32, 257 and 32769 (4.5e-7 ; 3.2e-5 against 3 x (9.9e-8 ; 1.2e-6), over by up to 1.5e-7; a build with libm activations stood there too), and the fp32
MFMA integrator on A `forward` (1.7e-7 ; 5.9e-6 against one ulp ; 3 x 1.9e-6).  A float32 evaluation that sums each layer term by term, the order of that
accumulator, gives 4.0e-7 ; 2.5e-5 and 2.0e-7 ; 6.3e-6 on the CPU for the same cases: the floor of vel, vel_gated and integrate is the worse of the two orders.
The file takes about 5 s on an MI355X; no test over 1 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import alpha64 as a64
import point64 as p64
from helpers import field_state, make_model

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
TAIL = 4096
MODES = ("x6", "fp32")
N_BIG = p64.SIZES[-1]


@pytest.fixture(scope="module")
def dev():
    """fields A, B and D: the device module and the yardstick's field of the same parameters"""
    from test_gpu_charloss import sh_model
    out = {}
    for kind in p64.KINDS:
        model = sh_model() if kind == "D" else make_model(kind)[0]
        model.eval()
        out[kind] = (model.nvfi, p64.field_of(*field_state(model), sh=kind == "D"))
    return out


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _published(f, name, N, times=1):
    from nvfi_amd import _lib
    nb = C.c_int64(0)
    _lib.check(getattr(_lib.lib(), name)(C.byref(f._desc()), C.c_int64(N), C.byref(nb)))
    return times * int(nb.value)


def _guarded(call, nb, outs, label):
    """`call(ws, nbytes)` with exactly the published size and a tail of 0xA5 behind it, then with 256 bytes less into fresh sentinels: (4), and
    neither an output nor a workspace byte changes.  Returns the outputs of the good call."""
    ws = torch.full((nb + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    good = [torch.full(s, SENTINEL, device="cuda") for s in outs]
    assert call(ws, nb, *good) == 0, label
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xA5).all()), (label, "the call wrote behind the size it publishes")
    ws2 = torch.full((nb + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    bad = [torch.full(s, SENTINEL, device="cuda") for s in outs]
    assert call(ws2, nb - 256, *bad) == 4, (label, "an undersized workspace is not refused")
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bad) and bool((ws2 == 0x5A).all()), (label, "a refused call wrote something")
    return good


def _lib():
    from nvfi_amd import _lib as L
    return L


def c_vel_eval(f, xt, gated, desc=None):
    L = _lib()
    d = f._desc() if desc is None else desc
    return lambda ws, nb, u: L.lib().nvfi_vel_eval(C.byref(d), C.c_int64(xt.shape[0]), L.ptr(xt), L.ptr(u), C.c_int(int(gated)), L.ptr(ws), C.c_int64(nb), _stream())


def c_integrate(f, x, t, base, desc=None):
    L = _lib()
    d = f._desc() if desc is None else desc
    return lambda ws, nb, xk: L.lib().nvfi_integrate_pos(C.byref(d), C.c_int64(x.shape[0]), L.ptr(x), L.ptr(t), L.ptr(base), L.ptr(xk), L.ptr(ws), C.c_int64(nb), _stream())


def c_app_at(f, q, view):
    L = _lib()
    d = f._desc()
    return lambda ws, nb, rgb: L.lib().nvfi_app_at(C.byref(d), C.c_int64(q.shape[0]), L.ptr(q), L.ptr(view), L.ptr(rgb), L.ptr(ws), C.c_int64(nb), _stream())


def c_render_mlp(f, x3, view, feat):
    L = _lib()
    d = f._desc()
    return lambda ws, nb, rgb: L.lib().nvfi_render_mlp(C.byref(d), C.c_int64(x3.shape[0]), L.ptr(x3), L.ptr(view), L.ptr(feat), L.ptr(rgb), L.ptr(ws), C.c_int64(nb), _stream())


def density_at(f, q):
    L = _lib()
    N = q.shape[0]
    feat, sigma = torch.full((N,), SENTINEL, device="cuda"), torch.full((N,), SENTINEL, device="cuda")
    L.check(L.lib().nvfi_density_at(C.byref(f._desc()), C.c_int64(N), L.ptr(q), L.ptr(feat), L.ptr(sigma), _stream()))
    return feat, sigma


def held(label, key, got, ref, keep=None):
    """prints the device's figures next to the bound and returns the excess over it (<= 0: every element inside)"""
    rtol, atol = p64.POINT_RTOL[key], p64.POINT_ATOL[key]
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if keep is not None:
        got, ref = got[keep], ref[keep]
    da, dr = a64.floors(got, ref) if ref.size else (0.0, 0.0)
    e = p64.excess(got, ref, rtol, atol)
    fa, fr = p64.FLOOR[key]
    print(f"[point64] {label}: device abs {da:.2e} rel {dr:.2e} | bound atol {atol:g} rtol {rtol:g} [float32 {fa:.1e} ; {fr:.1e}] | excess {e:.1e}", flush=True)
    return e


class _mode:
    """the field's integrator for the block: "x6" (the default) or "fp32" (vel_fp16 bit 3: the fp32 MFMA kernels)"""

    def __init__(self, f, mode):
        self.f, self.mode = f, mode

    def __enter__(self):
        self.keep = self.f.vel_fp16
        if self.mode == "fp32":
            self.f.vel_fp16 = "fp32"
        assert bool(self.f._desc().vel_fp16 & 8) == (self.mode == "fp32")

    def __exit__(self, *a):
        self.f.vel_fp16 = self.keep


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("N", p64.SIZES)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_vel_eval(dev, kind, N):
    f, fld = dev[kind]
    xt = p64.case_points(fld, N, "vel")
    xd = _cu(xt)
    nb = _published(f, "nvfi_vel_workspace_bytes", N)
    bad = []
    # ---- un-gated: (v, a)
    ref = p64.vel64(fld, xt, False, device="cuda")
    u, = _guarded(c_vel_eval(f, xd, 0), nb, [(N, 6)], (kind, N, "vel"))
    if held(f"vel:{kind}:N{N}", ("vel", kind, "all"), u.cpu().numpy(), ref["u"]) > 0:
        bad.append("vel")
    w = f.vel_net(xd)
    assert w.shape == (N, 6) and torch.equal(w, u)
    # ---- gated: v inside the gate, exact zeros outside; columns 3-5 of the buffer are not the call's
    ref = p64.vel64(fld, xt, True, device="cuda")
    u, = _guarded(c_vel_eval(f, xd, 1), nb, [(N, 6)], (kind, N, "vel gated"))
    assert bool((u[:, 3:] == SENTINEL).all()), "the gated call wrote the acceleration columns"
    got = u[:, :3].cpu().numpy()
    edge = ref["edge"].copy()
    if N >= 31:
        assert edge[:p64.N_FACE].all()
        edge[:p64.N_FACE] = False         # ON the box: both sides compare the same two fp32 numbers
    assert edge.sum() <= int(0.005 * N)
    assert np.array_equal((got == 0)[~edge], (ref["u"] == 0)[~edge]), (kind, N, "the zero pattern of the gate")
    assert np.isfinite(got).all()
    if held(f"vel_gated:{kind}:N{N}", ("vel_gated", kind, "all"), got, ref["u"], ~edge) > 0:
        bad.append("vel_gated")
    g = f.vel(xd)
    assert g.shape == (N, 3) and torch.equal(g, u[:, :3])
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (b)
def _check_positions(label, key, got, ref, fld):
    """the bound off the near-face points; those are printed, finite and inside 1.2 x the gate box"""
    edge = ref["edge"]
    e = held(label, key, got, ref["xk"], ~edge)
    if edge.any():
        print(f"[point64] {label}: near-face points {np.nonzero(edge)[0].tolist()}: device {got[edge]}, yardstick {ref['xk'][edge]}")
        c, h = p64._gate(fld)
        assert np.isfinite(got[edge]).all() and (np.abs(got[edge] - c) <= 1.2 * h).all()
    return e


@pytest.mark.parametrize("N", p64.SIZES)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_integrate_pos(dev, kind, N):
    f, fld = dev[kind]
    x = p64.case_points(fld, N, "pos")
    xd = _cu(x)
    nb = _published(f, "nvfi_vel_workspace_bytes", N)
    bad = []
    for label in p64.TIME_CASES:
        if N not in p64.case_sizes(label):
            continue
        t, base = p64.time_cases(fld, N, label)
        td, bd = _cu(t), _cu(base)
        ref = p64.integrate64(fld, x, t, base, device="cuda")
        assert ref["edge"].sum() <= int(0.005 * N), (label, int(ref["edge"].sum()))
        if label == "mixed" and N >= 257:
            assert (t > base).any() and (t < base).any() and (t > fld.tmax).any(), "both signs, and extrapolation beyond tmax"
            assert (ref["n_rejected"] > 0) == (kind == "B")
        key = ("integrate", kind, label)
        for mode in MODES:
            with _mode(f, mode):
                x0, t0, b0 = xd.clone(), td.clone(), bd.clone()
                got_t = f.integrate_pos(xd, td, bd)
                assert torch.equal(xd, x0) and torch.equal(td, t0) and torch.equal(bd, b0), (label, mode, "the wrapper changed its arguments")
                assert got_t.shape == (N, 3)
                got = got_t.cpu().numpy()
                tag = f"integrate:{kind}:{label}:N{N}:{mode}"
                print(f"[point64] {tag}: steps per point up to {int(ref['steps'].max())}, {int(ref['steps'].sum())} in all, {ref['n_rejected']} rejected")
                if _check_positions(tag, key, got, ref, fld) > 0:
                    bad.append((label, mode))
                if label == "none":
                    assert torch.equal(got_t, xd), (mode, "t == base moved a point")
                if label == "one_live":
                    still = np.ones(N, bool)
                    still[p64.one_live_points(N)] = False
                    assert np.array_equal(got[still], x[still]), (mode, "a point with t == base moved beside a live one")
                if label == "mixed":
                    # (h) the published size, and the other argument forms of the wrapper: the same bits
                    xk, = _guarded(c_integrate(f, xd, td, bd), nb, [(N, 3)], (kind, N, mode, "integrate_pos"))
                    assert torch.equal(xk, got_t)
                    assert torch.equal(f.integrate_pos(xd, td[:, None], bd[:, None]), got_t), "(N, 1) times"
                    assert torch.equal(f.integrate_pos(xd.double(), td.double(), bd.double()), got_t), "float64 inputs"
                    wide = torch.cat([xd, xd[:, :1]], 1)
                    assert not wide[:, :3].is_contiguous() or N == 1
                    assert torch.equal(f.integrate_pos(wide[:, :3], td, bd), got_t), "a non-contiguous view"
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_integrate_pos_across_the_kernel_switch(dev, kind):
    import os
    env = {k: os.environ.get(k, d) for k, d in (("NVFI_X6W", "1"), ("NVFI_X6W_MIN_TILES", "4096"), ("NVFI_INTEGRATE_X6", "1"))}
    if env != {"NVFI_X6W": "1", "NVFI_X6W_MIN_TILES": "4096", "NVFI_INTEGRATE_X6": "1"}:
        pytest.skip(f"the two sizes sit either side of the kernel switch only under the default switches; got {env}")
    f, fld = dev[kind]
    x, t, base = p64.switch_inputs(fld, p64.SWITCH_N + 1)
    ref = p64.integrate64(fld, x, t, base, device="cuda")
    assert ref["edge"].sum() <= int(0.005 * p64.SWITCH_N)
    xd, td, bd = _cu(x), _cu(t), _cu(base)
    outs, bad = {}, []
    with _mode(f, "x6"):
        for N in (p64.SWITCH_N, p64.SWITCH_N + 1):
            outs[N] = f.integrate_pos(xd[:N].contiguous(), td[:N].contiguous(), bd[:N].contiguous())
            sub = dict(xk=ref["xk"][:N], edge=ref["edge"][:N])
            if _check_positions(f"integrate:{kind}:mixed:N{N}:x6", ("integrate", kind, "mixed"), outs[N].cpu().numpy(), sub, fld) > 0:
                bad.append(N)
    ndiff = int((outs[p64.SWITCH_N] != outs[p64.SWITCH_N + 1][:p64.SWITCH_N]).any(1).sum())
    print(f"[point64] switch:{kind}: points that differ between the four-wave and the one-wave-per-tile kernel: {ndiff} of {p64.SWITCH_N}")
    assert ndiff == 0 and not bad, (ndiff, bad)


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("N", p64.SIZES)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_density_at(dev, kind, N):
    f, fld = dev[kind]
    q = p64.case_points(fld, N, "density")
    qd = _cu(q)
    ref = p64.density64(fld, q, device="cuda")
    feat, sigma = density_at(f, qd)
    feat, sigma = feat.cpu().numpy(), sigma.cpu().numpy()
    nf = min(p64.N_FAR, max(0, N - len(p64.SPECIAL_T)))
    if nf:
        assert np.isfinite(q).all() and np.abs(q[N - nf:, :3]).min() >= 3.0
        assert (ref["feat"][N - nf:] == 0).all(), "the yardstick reads padding only at a far point"
        assert not feat[N - nf:].view(np.uint32).any(), ("a far point's feature is not +0.0 bit for bit", feat[N - nf:])
    e1 = held(f"feat:{kind}:N{N}", ("feat", kind, "all"), feat, ref["feat"])
    e2 = held(f"sigma:{kind}:N{N}", ("sigma", kind, "all"), sigma, ref["sigma"])
    w = f.compute_densityfeature(qd)
    assert w.shape == (N, 1) and np.array_equal(w[:, 0].cpu().numpy(), feat)
    assert e1 <= 0 and e2 <= 0, (e1, e2)


# ---------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("N", p64.SIZES)
@pytest.mark.parametrize("kind", p64.KINDS)
def test_app_at_and_render_mlp(dev, kind, N):
    f, fld = dev[kind]
    q, view, feat = p64.case_points(fld, N, "app")
    qd, vd, fd = _cu(q), _cu(view), _cu(feat)
    x3 = qd[:, :3].contiguous()
    nb = _published(f, "nvfi_app_workspace_bytes", N)
    bad = []
    ref = p64.app64(fld, q, view, device="cuda")
    rgb, = _guarded(c_app_at(f, qd, vd), nb, [(N, 3)], (kind, N, "app_at"))
    if held(f"app:{kind}:N{N}", ("app", kind, "all"), rgb.cpu().numpy(), ref["rgb"]) > 0:
        bad.append("app")
    assert torch.equal(f.app_at(qd, vd), rgb)
    refm = p64.mlp64(fld, q[:, :3], view, feat, device="cuda")
    rgbm, = _guarded(c_render_mlp(f, x3, vd, fd), 2 * nb, [(N, 3)], (kind, N, "render_mlp"))
    if held(f"mlp:{kind}:N{N}", ("mlp", kind, "all"), rgbm.cpu().numpy(), refm) > 0:
        bad.append("mlp")
    with torch.no_grad():
        assert torch.equal(f.renderModule(x3, vd, fd, {}) if kind != "D" else f._render_module_call(x3, vd, fd), rgbm)
    if kind != "D":
        for c in (rgb, rgbm):
            assert bool(((c >= 0) & (c <= 1)).all())
    else:
        s = f.sh_render(vd, fd)
        assert s.shape == (N, 3)
        if held(f"sh:{kind}:N{N}", ("sh", kind, "all"), s.cpu().numpy(), p64.sh64(view, feat, device="cuda")) > 0:
            bad.append("sh")
        if held(f"sh vs render_mlp:{kind}:N{N}", ("sh", kind, "all"), s.cpu().numpy(), rgbm.cpu().numpy().astype(np.float64)) > 0:
            bad.append("sh vs render_mlp")
        assert bool((s >= 0).all()) and bool((s == 0).any() or N < 31)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("kind", p64.KINDS)
def test_prefix_invariance(dev, kind):
    f, fld = dev[kind]
    q, view, feat = (_cu(a) for a in p64.case_points(fld, N_BIG, "app"))
    calls = {"app_at": lambda n: f.app_at(q[:n].contiguous(), view[:n].contiguous()),
             "render_mlp": lambda n: f._render_module_call(q[:n, :3].contiguous(), view[:n].contiguous(), feat[:n].contiguous())}
    if kind == "D":
        calls["sh_render"] = lambda n: f.sh_render(view[:n].contiguous(), feat[:n].contiguous())
    else:
        xt = _cu(p64.case_points(fld, N_BIG, "vel"))
        x = _cu(p64.case_points(fld, N_BIG, "pos"))
        t, base = (_cu(a) for a in p64.time_cases(fld, N_BIG, "mixed"))
        qd = _cu(p64.case_points(fld, N_BIG, "density"))
        calls["vel_eval"] = lambda n: f.vel_net(xt[:n].contiguous())
        calls["vel_eval gated"] = lambda n: f.vel(xt[:n].contiguous())
        calls["density_at feat"] = lambda n: density_at(f, qd[:n].contiguous())[0]
        calls["density_at sigma"] = lambda n: density_at(f, qd[:n].contiguous())[1]
        for mode in MODES:
            def run(n, mode=mode):
                with _mode(f, mode):
                    return f.integrate_pos(x[:n].contiguous(), t[:n].contiguous(), base[:n].contiguous())
            calls[f"integrate_pos {mode}"] = run
    bad = []
    with torch.no_grad():
        for name, call in calls.items():
            full = call(N_BIG)
            for n in p64.SIZES[:-1]:
                part = call(n)
                nd = int((part != full[:n]).reshape(n, -1).any(1).sum())
                if nd:
                    bad.append((name, n, nd))
            print(f"[point64] prefix:{kind}:{name}: sizes whose outputs differ from the first entries of the N = {N_BIG} call: {[b[1:] for b in bad if b[0] == name]}")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("kind", p64.KINDS)
def test_yardstick_sees_a_subtly_wrong_kernel(dev, kind):
    """nothing on the device is altered: its outputs are held against the yardstick's wrong variants and must leave the bound"""
    f, fld = dev[kind]
    N = 257
    seen = {}

    def see(name, key, got, wrong):
        e = p64.excess(got.cpu().numpy(), wrong, p64.POINT_RTOL[key], p64.POINT_ATOL[key])
        print(f"[point64] wrong:{kind}:{name}: the device is {e:.1e} over the bound of the wrong variant")
        seen[name] = seen.get(name, False) or e > 0

    q, view, feat = p64.case_points(fld, N, "app")
    qd, vd, fd = _cu(q), _cu(view), _cu(feat)
    see("app", ("app", kind, "all"), f.app_at(qd, vd), p64.app64(fld, q, view, device="cuda", wrong=True)["rgb"])
    see("mlp", ("mlp", kind, "all"), f._render_module_call(qd[:, :3].contiguous(), vd, fd), p64.mlp64(fld, q[:, :3], view, feat, device="cuda", wrong=True))
    if kind == "D":
        see("sh", ("sh", kind, "all"), f.sh_render(vd, fd), p64.sh64(view, feat, device="cuda", wrong=True))
    else:
        xt = p64.case_points(fld, N, "vel")
        see("vel", ("vel", kind, "all"), f.vel_net(_cu(xt)), p64.vel64(fld, xt, False, device="cuda", wrong=True)["u"])
        qq = p64.case_points(fld, N, "density")
        w = p64.density64(fld, qq, device="cuda", wrong=True)
        feat_d, sigma_d = density_at(f, _cu(qq))
        see("density", ("feat", kind, "all"), feat_d, w["feat"])
        see("density", ("sigma", kind, "all"), sigma_d, w["sigma"])
        x = p64.case_points(fld, N, "pos")
        for label in ("mixed", "forward", "one_live"):
            t, base = p64.time_cases(fld, N, label)
            w = p64.integrate64(fld, x, t, base, device="cuda", wrong=True)
            for mode in MODES:
                with _mode(f, mode):
                    see(f"integrate {mode}", ("integrate", kind, label), f.integrate_pos(_cu(x), _cu(t), _cu(base)), w["xk"])
    assert all(seen.values()), ("a bound does not see its wrong variant", seen)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_use_vel_0_is_refused(dev):
    """harmless without the guard as well: the descriptor is field A's, every weight pointer valid, only use_vel is cleared"""
    L = _lib()
    f, fld = dev["A"]
    N = 33
    xt = _cu(p64.case_points(fld, N, "vel"))
    d = f._desc()
    d.use_vel = 0
    nb = _published(f, "nvfi_vel_workspace_bytes", N)
    ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device="cuda")
    u = torch.full((N, 6), SENTINEL, device="cuda")
    for gated in (0, 1):
        assert c_vel_eval(f, xt, gated, d)(ws, nb, u) == 2 and "use_vel" in L.lib().nvfi_last_error().decode()
    x, t = xt[:, :3].contiguous(), xt[:, 3].contiguous()
    xk = torch.full((N, 3), SENTINEL, device="cuda")
    assert c_integrate(f, x, t, torch.zeros_like(t), d)(ws, nb, xk) == 2 and "use_vel" in L.lib().nvfi_last_error().decode()
    torch.cuda.synchronize()
    assert bool((u == SENTINEL).all()) and bool((xk == SENTINEL).all()) and bool((ws == 0xA5).all())
    m, _ = make_model("A", use_vel=False)
    with pytest.raises(L.NvfiError, match="use_vel"):
        m.nvfi.integrate_pos(x, t, torch.zeros_like(t))
    with pytest.raises(L.NvfiError, match="use_vel"):
        m.nvfi._vel_eval(xt, True)
