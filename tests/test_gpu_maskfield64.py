"""MaskField on the device - nvfi_maskfield_fwd / nvfi_maskfield_bwd through the C ABI (csrc/mask.hip: k_maskfield_fwd / _bwd and their fp16-input
twins; csrc/wgrad_ring.hip + k_wgrad_reduce for the weight gradients) - against its float64 restatement tests/maskfield64.py, which
tests/test_maskfield64_golden.py pins to the reference's goldens, at every class count the library accepts and at the tile edges.

Matrix (maskfield64.MATRIX): every K = 1..32 at N = 129; K in {2, 8, 17, 32} x N in {1, 31, 32, 33, 127, 128, 129, 8192, 8193, 16385} (the 32-point
wave tile, the 128-point workgroup, 256 / 257 tiles where the ring's 256 slab owners go from one tile each to one owner with two, two each and one
more); the steep heads (x 32: saturated softmax, probabilities that underflow) at K in {8, 17, 32}, N = 129.  From K = 9 on, accumulator registers
4..15 of the logit tile carry live rows; from K = 17 on both half-waves hold rows >= 8.
Per cell, through ctypes so that every output sits between two bands of 64 sentinel floats (bands untouched; no entry of the mask left at the sentinel;
the workspace is the published size with a 4 KiB tail that stays untouched):
  mask          max |device - float64| <= max(3 x d32, 5e-7), rows sum to 1 within 1e-6
  gradients     conftest.assert_grad against float64 under max(3 x d32, maskfield64.FLOOR_G) per tensor
  accumulation  the ten gradient buffers start from a pattern of signed powers of two, 2^e (1, 1/2, 1/4, 1/8 in turn), 2^e the power of two under the
                rms of the yardstick's tensor (so that the one fp32 rounding of `pattern + gradient` stays at rounding level of the gradient while an
                overwrite instead of an add would move the result by ~the gradient's own size); result - pattern is what is compared, and a second
                backward on the same workspace gives pattern + 2 x the gradient within the same bound
  K = 1         the mask is 1.0 and every gradient buffer the start pattern, bit for bit
  gate flips    N > 129 only, and only where the comparison above misses: the large cells hold points with a hidden unit within fp32 rounding of its
                kink (1.1 - 1.4 % of the points), where either side of the gate is a correct fp32 MaskField and the gradient jumps.
                maskfield64.admit_flips names the listed gates the device took the other way than float64, the yardstick is moved by exactly those,
                and the bound stays what it was.  The device does so in one cell: K = 8, N = 16385, point 5592, layer 1, unit 17 (z = 3.3e-8 in
                float64, 3e-3 rounding bounds from zero): without it point_fc.1.weight sits 4.7e-3 off, with it 3.2e-7.
d32 is the float32 evaluation of the yardstick against its float64 evaluation on the cell itself (float64 on the GPU in torch, float32 on the CPU);
no bound is taken from the device.  Every comparison prints error / bound; the worst ratios are printed when the module ends.

Further: the module route (MaskField(mask_dim=17) loaded with params_for(17) gives the ABI route's mask bits); partial gradient sets (biases only,
weights only, layer 4 only: the members given carry the bits of the full call, the others and every band stay as they were); two forward + backward
runs at K = 32, N = 8193 from identical start buffers give identical bits (the MLP weight gradients are order-independent on
one stream); refusals (2: mask_dim 0 and 33, n_dim 64, a NULL weight pointer; 4: a workspace one byte short, forward train and non-train, and a
backward on a workspace sized for a non-train forward - outputs left as they were; N = 0 returns 0 and writes nothing).
fp16-input mode (NVFI_MASK_FP16) at K in {9, 17, 32}, N in {33, 129}: against helpers.maskfield_fp16_oracle, a numpy restatement in the SAME
arithmetic (fp16-rounded MFMA operands, fp32 accumulation), under the tolerances of test_maskfield.py::test_gpu_maskfield_fp16_mfma_mode (mask rtol
2e-4, atol 2e-6; gradients < 1e-3) on kink-free points.  This is NOT a float64 comparison: it pins the rows >= 8 of the 16-bit kernels to an fp32
oracle of their own arithmetic.

Figures: worst over the cells of a group; bound = max(3 x [float32 evaluation, CPU], floor); floor 5e-7 (mask, abs), FLOOR_G = 9.3e-6 (gradients,
max(maxrel, rel_l2); 3 x 3.1e-6, the largest float32 figure of the matrix: mask_fc.bias at K = 2, N = 8193).
  group               mask [float32] / device     gradients [float32] / device (first = second backward to the printed digit)
  K 1-8    N <= 129   [9.3e-8] / 7.5e-8           [2.8e-6] / 1.4e-6
  K 1-8    N > 129    [1.1e-7] / 1.1e-7           [3.0e-6] / 1.3e-6      (K = 8, N = 16385 with the one gate admitted; 4.7e-3 without)
  K 9-16   N = 129    [3.4e-8] / 3.4e-8           [6.0e-7] / 5.0e-7
  K 17-32  N <= 129   [1.8e-8] / 2.0e-8           [6.0e-7] / 5.4e-7
  K 17-32  N > 129    [2.5e-8] / 2.8e-8           [5.8e-7] / 4.3e-7
  steep    N = 129    [1.7e-6] / 1.3e-6           [2.5e-6] / 5.8e-6      (0.63 of its bound: mask_fc.bias, K = 17; mask 0.48 of its bound, K = 8)
Row sums within 3.1e-7 of 1.  fp16-input mode against its own-arithmetic oracle: mask 6.5e-6 abs, gradients <= 1.3e-4.  No kernel changed.
Two mutations that only skip work, each built and run once: the store loop of k_maskfield_fwd stopping at register 8 (rows >= 16 never stored)
failed 41 of the 83 tests here (36 cells, the module route, the three partial sets, the repeat); k_wgrad_reduce dropping the last output row of a head
wider than 8 failed 51 (44 cells, the six fp16 cases, the module route); tests/test_maskfield.py passed on both.
The file takes about 8 s on an MI355X; no test over 1 s but the first, which loads the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import maskfield64 as m64
from conftest import assert_grad

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
BAND = 64
TAIL = 4096
TRAIN, FP16 = 1, 2
CELLS = [pytest.param(K, N, steep, id=f"K{K}-N{N}" + ("-steep" if steep else "")) for K, N, steep in m64.MATRIX]
WORST = {}           # quantity -> (error / bound, cell)


def _L():
    from nvfi_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class Guarded:
    """a float buffer between two bands of BAND sentinel floats"""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, device="cuda")
        self.t = self.buf[BAND:BAND + n].view(*shape) if n else self.buf[BAND:BAND]
        if fill is not None and n:
            self.t.copy_(_cu(fill))

    def bands_intact(self):
        return bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[self.buf.numel() - BAND:] == SENTINEL).all())

    def numpy(self):
        return self.t.detach().cpu().numpy().copy()


def pattern(ref):
    """the start of a gradient buffer: +-2^e (1, 1/2, 1/4, 1/8), 2^e the power of two under the rms of the yardstick's tensor (1 where that is zero)"""
    ref = np.asarray(ref, np.float64)
    rms = float(np.sqrt((ref ** 2).mean())) if ref.size else 0.0
    scale = 2.0 ** np.floor(np.log2(rms)) if rms > 0 else 1.0
    i = np.arange(ref.size)
    return (scale * np.where((i // 4) % 2 == 0, 1.0, -1.0) * 2.0 ** -(i % 4)).astype(np.float32).reshape(ref.shape)


def desc(dev_params, K, n_layer=4, n_dim=128):
    L = _L()
    md = L.MaskDesc()
    md.n_layer, md.n_dim, md.mask_dim = n_layer, n_dim, K
    for i in range(5):
        md.W[i] = L.ptr(dev_params[2 * i]); md.b[i] = L.ptr(dev_params[2 * i + 1])
    return md


def published(md, N, train):
    L = _L()
    nb = C.c_int64(-1)
    assert L.lib().nvfi_maskfield_workspace_bytes(C.byref(md), C.c_int64(N), C.c_int(train), C.byref(nb)) == 0
    return int(nb.value)


def fwd(md, N, x, out, mode, ws, nbytes):
    L = _L()
    return L.lib().nvfi_maskfield_fwd(C.byref(md), C.c_int64(N), L.ptr(x), L.ptr(out), C.c_int(mode), L.ptr(ws), C.c_int64(nbytes), _stream())


def bwd(md, N, g, grads, mode, ws, nbytes, members=range(10)):
    """grads: ten tensors in maskfield64.GRAD_KEYS order (W0, b0, ...); members: the indices handed to the library, the others go in as NULL"""
    L = _L()
    mg = L.MaskGrads()
    for l in range(5):
        mg.W[l] = L.ptr(grads[2 * l]) if 2 * l in members else None
        mg.b[l] = L.ptr(grads[2 * l + 1]) if 2 * l + 1 in members else None
    return L.lib().nvfi_maskfield_bwd(C.byref(md), C.c_int64(N), L.ptr(g), C.byref(mg), C.c_int(mode), L.ptr(ws), C.c_int64(nbytes), _stream())


class Run:
    """one training forward and `repeats` backwards of a cell through the ABI, every output guarded; .mask, .grads[r][key] (numpy, fp32 bits)"""

    def __init__(self, p, x, g, start, mode=TRAIN, repeats=1, members=range(10)):
        N, K = x.shape[0], p[8].shape[0]
        self.dev = [_cu(a) for a in p]
        self.md = desc(self.dev, K)
        self.nb = published(self.md, N, 1)
        self.ws = torch.full((self.nb + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out = Guarded((N, K))
        self.bufs = [Guarded(a.shape, a) for a in start]
        xd, gd = _cu(x), _cu(g)
        assert fwd(self.md, N, xd, self.out.t, mode, self.ws, self.nb) == 0, _L().lib().nvfi_last_error()
        self.grads = []
        for _ in range(repeats):
            assert bwd(self.md, N, gd, [b.t for b in self.bufs], mode, self.ws, self.nb, members) == 0, _L().lib().nvfi_last_error()
            self.grads.append({k: b.numpy() for k, b in zip(m64.GRAD_KEYS, self.bufs)})
        torch.cuda.synchronize()
        self.mask = self.out.numpy()
        assert bool((self.ws[self.nb:] == 0xA5).all()), "a call wrote behind the workspace size it publishes"
        assert self.out.bands_intact(), "mask_out: a band was written"
        for k, b in zip(m64.GRAD_KEYS, self.bufs):
            assert b.bands_intact(), (k, "a band was written")
        assert not (self.mask == SENTINEL).any(), "an entry of mask_out was never written"


def _note(quantity, e, bound, cell):
    r = e / bound
    if r > WORST.get(quantity, (-1.0, None))[0]:
        WORST[quantity] = (r, cell)
    return r


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for q, (r, cell) in sorted(WORST.items()):
        print(f"[maskfield64] worst error / bound, {q}: {r:.3f} at {cell}", flush=True)


_starts = {}


def start_of(K, N, steep, device="cuda"):
    """(y64, bound, start buffers) of a cell"""
    key = (K, N, steep)
    if key not in _starts:
        y64, _, bound = m64.yardstick(K, N, steep, device=device)
        _starts[key] = (y64, bound, [pattern(y64[k]) for k in m64.GRAD_KEYS])
    return _starts[key]


@pytest.mark.parametrize("K,N,steep", CELLS)
def test_matrix(K, N, steep):
    cell = f"K{K} N{N}" + (" steep" if steep else "")
    p, x, g = m64.case(K, N, steep)
    y64, bound, start = start_of(K, N, steep)
    run = Run(p, x, g, start, repeats=2)
    assert run.mask.shape == (N, K) and run.mask.dtype == np.float32
    if K == 1:
        assert (run.mask == 1.0).all(), cell
        for r in run.grads:
            for k, s in zip(m64.GRAD_KEYS, start):
                assert np.array_equal(r[k].view(np.uint32), s.view(np.uint32)), (cell, k, "K = 1: the gradient is exactly zero")
        return
    e = float(np.abs(run.mask.astype(np.float64) - y64["mask"]).max())
    rs = float(np.abs(run.mask.astype(np.float64).sum(1) - 1.0).max())
    print(f"[maskfield64] {cell}: mask {e:.2e} / {bound['mask']:.2e} = {_note('mask', e, bound['mask'], cell):.3f}; row sums off by {rs:.1e}", flush=True)
    assert e <= bound["mask"], (cell, "mask", e, bound["mask"])
    assert rs <= 1e-6, (cell, "row sums", rs)
    assert (run.mask >= 0).all()
    ref = y64
    first = {k: run.grads[0][k].astype(np.float64) - s.astype(np.float64) for k, s in zip(m64.GRAD_KEYS, start)}
    if N > 129 and any(m64.err(first[k], y64[k]) > bound[k] for k in m64.GRAD_KEYS):
        # a large cell holds gates within fp32 rounding of their kink (maskfield64.KINK_CAP); either side is a correct fp32 MaskField
        ref, taken = m64.admit_flips(first, y64, m64.gate_flips(p, x, g))
        print(f"[maskfield64] {cell}: gates the device took the other way than float64 (point, layer, unit, rounding bounds from zero): {taken}", flush=True)
    for rep, q in ((1, "gradient"), (2, "second backward")):
        line = []
        for k, s in zip(m64.GRAD_KEYS, start):
            got = run.grads[rep - 1][k].astype(np.float64) - s.astype(np.float64)
            ge = m64.err(got, rep * ref[k])
            line.append(f"{k} {ge:.1e}/{bound[k]:.1e}")
            _note(q, ge, bound[k], f"{cell} {k}")
            assert_grad(got, rep * ref[k], bound[k], label=f"{cell} {k} x{rep}")
        print(f"[maskfield64] {cell}: {q}: " + ", ".join(line), flush=True)


def test_module_route():
    from nvfi_amd.models import MaskField
    K, N = 17, 129
    p, x, g = m64.case(K, N)
    y64, bound, start = start_of(K, N, False)
    run = Run(p, x, g, start)
    mf = MaskField(mask_dim=K)
    mf.load_state_dict({k: torch.from_numpy(a) for k, a in zip(m64.GRAD_KEYS, p)})
    mf = mf.cuda()
    mask = mf(_cu(x))
    assert np.array_equal(mask.detach().cpu().numpy().view(np.uint32), run.mask.view(np.uint32))
    with torch.no_grad():
        assert torch.equal(mf(_cu(x)), mask.detach())                      # the non-train forward
    (mask * _cu(g)).sum().backward()
    for k, s in zip(m64.GRAD_KEYS, start):                                 # (the module adds into zeros, the ABI run into the pattern: not the same bits)
        assert_grad(mf.get_parameter(k).grad.cpu().numpy(), y64[k], bound[k], label=f"module {k}")


SETS = {"biases": (1, 3, 5, 7, 9), "weights": (0, 2, 4, 6, 8), "layer4": (8, 9)}


@pytest.mark.parametrize("which", sorted(SETS))
def test_partial_gradient_sets(which):
    K, N = 17, 129
    p, x, g = m64.case(K, N)
    _, _, start = start_of(K, N, False)
    full = Run(p, x, g, start)
    part = Run(p, x, g, start, members=SETS[which])
    assert np.array_equal(part.mask.view(np.uint32), full.mask.view(np.uint32))
    for i, (k, s) in enumerate(zip(m64.GRAD_KEYS, start)):
        want = full.grads[0][k] if i in SETS[which] else s
        assert np.array_equal(part.grads[0][k].view(np.uint32), want.view(np.uint32)), (which, k, "given: the full call's bits; not given: untouched")
        assert (i not in SETS[which]) or not np.array_equal(want, s), (which, k, "the full call left the pattern unchanged")


def test_repeats_bit_for_bit():
    K, N = 32, 8193
    p, x, g = m64.case(K, N)
    _, _, start = start_of(K, N, False)
    a, b = Run(p, x, g, start), Run(p, x, g, start)
    assert np.array_equal(a.mask.view(np.uint32), b.mask.view(np.uint32))
    for k in m64.GRAD_KEYS:
        assert np.array_equal(a.grads[0][k].view(np.uint32), b.grads[0][k].view(np.uint32)), k


def test_refusals():
    L = _L()
    K, N = 8, 33
    p, x, g = m64.case(K, N)
    dev = [_cu(a) for a in p]
    xd, gd = _cu(x), _cu(g)
    start = [pattern(np.ones_like(a)) for a in p]
    good = desc(dev, K)
    nb1, nb0 = published(good, N, 1), published(good, N, 0)
    assert 0 < nb0 < nb1
    ws = torch.full((nb1 + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    out = Guarded((N, K))
    bufs = [Guarded(a.shape, a) for a in start]

    def untouched(label):
        torch.cuda.synchronize()
        assert bool((out.buf == SENTINEL).all()), (label, "mask_out was written")
        for k, b, s in zip(m64.GRAD_KEYS, bufs, start):
            assert b.bands_intact() and np.array_equal(b.numpy().view(np.uint32), s.view(np.uint32)), (label, k, "a gradient buffer was written")
        assert bool((ws == 0xA5).all()), (label, "the workspace was written")

    bad = {"mask_dim 0": desc(dev, 0), "mask_dim 33": desc(dev, 33), "n_dim 64": desc(dev, K, n_dim=64), "NULL weight": desc(dev[:4] + [None] + dev[5:], K)}
    for label, md in bad.items():
        nb = C.c_int64(-1)
        assert L.lib().nvfi_maskfield_workspace_bytes(C.byref(md), C.c_int64(N), C.c_int(1), C.byref(nb)) == 2 and nb.value == -1, label
        assert fwd(md, N, xd, out.t, TRAIN, ws, nb1) == 2, label
        assert L.lib().nvfi_last_error(), label
        assert bwd(md, N, gd, [b.t for b in bufs], TRAIN, ws, nb1) == 2, label
        untouched(label)
    assert fwd(good, N, xd, out.t, TRAIN, ws, nb1 - 1) == 4
    assert fwd(good, N, xd, out.t, 0, ws, nb0 - 1) == 4
    untouched("a workspace one byte short, forward")
    assert bwd(good, N, gd, [b.t for b in bufs], TRAIN, ws, nb1 - 1) == 4
    untouched("a workspace one byte short, backward")
    assert fwd(good, 0, xd, out.t, TRAIN, ws, nb1) == 0 and bwd(good, 0, gd, [b.t for b in bufs], TRAIN, ws, nb1) == 0
    untouched("N = 0")
    # a non-train forward in its own published size works, and the backward refuses that workspace
    ws0 = torch.full((nb0 + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    assert fwd(good, N, xd, out.t, 0, ws0, nb0) == 0
    assert bwd(good, N, gd, [b.t for b in bufs], 0, ws0, nb0) == 4
    torch.cuda.synchronize()
    assert bool((ws0[nb0:] == 0xA5).all()) and out.bands_intact() and not (out.numpy() == SENTINEL).any()
    for k, b, s in zip(m64.GRAD_KEYS, bufs, start):
        assert b.bands_intact() and np.array_equal(b.numpy().view(np.uint32), s.view(np.uint32)), k
    y = m64.mask64(p, x)["mask"]
    assert np.abs(out.numpy() - y).max() <= m64.MASK_FLOOR


@pytest.mark.parametrize("N", [33, 129])
@pytest.mark.parametrize("K", [9, 17, 32])
def test_fp16_input_mode(K, N):
    """NOT a float64 comparison: the fp16-input kernels against an fp32 oracle of the same arithmetic (see the module docstring)"""
    from helpers import maskfield_fp16_oracle
    p, x, g = m64.case(K, N)
    omask, ograds = maskfield_fp16_oracle(p, x, g)
    start = [np.zeros_like(a) for a in p]
    run = Run(p, x, g, start, mode=TRAIN | FP16)
    np.testing.assert_allclose(run.mask, omask, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(run.mask.sum(1), 1.0, atol=1e-5)
    line = []
    for k, og in zip(m64.GRAD_KEYS, ograds):
        e = m64.err(run.grads[0][k], og)
        line.append(f"{k} {e:.1e}")
        assert e < 1e-3, (K, N, k, e)
    print(f"[maskfield64] fp16-input K{K} N{N}: mask {np.abs(run.mask - omask).max():.1e} abs; gradients vs the same-arithmetic oracle: " + ", ".join(line))
