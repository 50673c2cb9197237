"""Float64 restatement of MaskField on free points (include/nvfi_hip.h: nvfi_maskfield_fwd / nvfi_maskfield_bwd; the reference's
models/mask_field.py:68-83 as train_segm.py:97-102 builds it), forward and parameter gradients, at every class count the library accepts:

  mask(x) = softmax(W4 relu(W3 relu(W2 relu(W1 relu(W0 x + b0) + b1) + b2) + b3) + b4),  3 -> 128 x 4 -> K,  1 <= K <= 32
  with g (N, K) = d loss / d mask: the ten gradients of (mask * g).sum() with respect to W0, b0, ..., W4, b4; the points carry none.

The yardstick of tests/test_maskfield64_golden.py (CPU: against the reference's goldens, and what a cut kernel would move) and of
tests/test_gpu_maskfield64.py (the device).  Plain torch, any device.  The parameters' VALUES and the points are fp32 numbers on both sides; everything
else runs in `dtype`.  dtype=float32 is "a plain fp32 implementation" of the same statement: its distance from the float64 run is the noise floor the
bounds of both files are derived from, computed on the case itself.

Parameters (params_for): the trunk is the four point_fc layers of tests/golden/maskfield.npz, tag K8, for every K.  The head for K <= 8 is the first
K rows of the K8 head (tests/test_gpu_objects.py builds K = 5 so); for K > 8 rows 0..7 of the K8 head followed by rows drawn from
np.random.default_rng(1000 + K), uniform in +- the K8 head's own max |w| (weights) and max |b| (biases).  steep=True multiplies the head's weight and
bias by 32: the softmax saturates and some probabilities underflow in fp32.

Points (points): uniform in [-1, 1]^3, g standard normal, fp32, from np.random.default_rng(seed).  A ReLU whose pre-activation lies within rounding of
zero may open in one fp32 evaluation and stay shut in another, and the point's gradient jumps there: margin() measures, per point, how many fp32
rounding bounds the nearest of the 512 hidden pre-activations stays away from zero.  For N <= 129 a point with margin < 4 is redrawn, so the small
cases sit away from every kink; larger cases stay as drawn, and at most KINK_CAP of their points may have margin < 1 (asserted by the golden test).
On those points an fp32 evaluation may take the other side of a gate than float64 does, and both are correct fp32 MaskFields: gate_flips lists every
such gate with what it changes, admit_flips finds the ones a result took the other way (the device at K = 8, N = 16385: point 5592, layer 1,
unit 17, z = 3.3e-8 in float64, 3e-3 rounding bounds from zero; that one gate moves point_fc.0 / point_fc.1 by 6e-4 .. 5e-3 of their peaks and,
once admitted, leaves 3.6e-7).

Bounds (bounds): never from the device.  Gradients, max(maxrel, rel_l2) per tensor: max(3 x d32, FLOOR_G), d32 the float32 evaluation's distance from
the float64 one on the same case; 3 is the project's headroom for another summation order (render64, raydist64).  FLOOR_G only keeps a tensor whose
own fp32 figure happens to be ~1e-7 from getting a bound below what another order of the same sums may cost: 3 x the largest d32 of the whole
matrix, measured on the CPU (MAX_D32; the golden test measures it again).  Mask, max absolute error: max(3 x d32, MASK_FLOOR), MASK_FLOOR = 5e-7 =
4 ulp of 1.0: one for expf, one for the division, the rest for the 128-term logit sum."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLD, maxrel, rel_l2
from objects64 import mask_field

NAMES = ["point_fc.0", "point_fc.1", "point_fc.2", "point_fc.3", "mask_fc"]
GRAD_KEYS = [f"{n}.{s}" for n in NAMES for s in ("weight", "bias")]            # the order of params_for / nvfi_mask_grads {W[l], b[l]}

# the matrix of tests/test_gpu_maskfield64.py (K, N, steep)
K_ALL = tuple(range(1, 33))
K_EDGE = (2, 8, 17, 32)
N_EDGE = (1, 31, 32, 33, 127, 128, 129, 8192, 8193, 16385)       # the 32-point wave tile, the 128-point workgroup, 256 / 257 tiles: the ring's 256 slab
K_STEEP = (8, 17, 32)                                            # owners go from one tile each to one owner with two; two tiles per owner and one more
N_SMALL = 129
MATRIX = ([(K, N_SMALL, False) for K in K_ALL] + [(K, N, False) for K in K_EDGE for N in N_EDGE if N != N_SMALL]
          + [(K, N_SMALL, True) for K in K_STEEP])

MASK_FLOOR = 5e-7
MAX_D32 = 3.1e-6          # largest max(maxrel, rel_l2) of a float32 gradient tensor against float64 over MATRIX, on the CPU, rounded up: 3.02e-6,
                          # mask_fc.bias at K = 2, N = 8193 (2.8e-6 mask_fc.weight at K = 2, N = 128; 2.5e-6 steep; every K >= 3 cell under 1.5e-6)
FLOOR_G = 3 * MAX_D32
KINK_MARGIN = 4.0
KINK_CAP = 0.025          # share of a large case's points that may sit within one rounding bound of a kink (measured 1.1 - 1.4 %)


def _gold():
    return np.load(os.path.join(GOLD, "maskfield.npz"))


def gold_params(tag, z=None):
    z = _gold() if z is None else z
    return [np.ascontiguousarray(z[f"{tag}:sd:{n}.{s}"], dtype=np.float32) for n in NAMES for s in ("weight", "bias")]


_params = {}


def params_for(K, steep=False):
    """[W0, b0, .., W4, b4] (fp32 numpy) of the class count K"""
    if not 1 <= K <= 32:
        raise ValueError(K)
    if (K, steep) not in _params:
        p = gold_params("K8")
        W, b = p[8], p[9]
        if K > 8:
            rng = np.random.default_rng(1000 + K)
            W = np.concatenate([W, rng.uniform(-1.0, 1.0, (K - 8, 128)).astype(np.float32) * np.abs(W).max()])
            b = np.concatenate([b, rng.uniform(-1.0, 1.0, K - 8).astype(np.float32) * np.abs(b).max()])
        W, b = W[:K], b[:K]
        if steep:
            W, b = W * np.float32(32.0), b * np.float32(32.0)
        _params[(K, steep)] = p[:8] + [np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)]
    return [a.copy() for a in _params[(K, steep)]]


def mask64(params, x, g=None, dtype=torch.float64, device="cpu"):
    """{mask (N, K)} and, with g (N, K), the ten gradients of (mask * g).sum() under GRAD_KEYS: numpy arrays of `dtype`"""
    ps = [torch.as_tensor(np.asarray(p, np.float32)).to(device=device, dtype=dtype).requires_grad_(g is not None) for p in params]
    xt = torch.as_tensor(np.asarray(x, np.float32)).to(device=device)
    with torch.set_grad_enabled(g is not None):
        mask = mask_field(ps, xt, dtype)
    out = {"mask": mask.detach().cpu().numpy()}
    if g is not None:
        gt = torch.as_tensor(np.asarray(g, np.float32)).to(device=device, dtype=dtype)
        grads = torch.autograd.grad((mask * gt).sum(), ps, allow_unused=True)
        for k, p, gr in zip(GRAD_KEYS, ps, grads):
            out[k] = (torch.zeros_like(p) if gr is None else gr).cpu().numpy()
    return out


def unit_margins(params, x):
    """four (N, 128) float64 arrays: |z| / ((n_in + 1) 6e-8 (|W||h| + |b|)) of every hidden pre-activation of every point"""
    h = torch.as_tensor(np.asarray(x, np.float32)).to(torch.float64)
    out = []
    for l in range(4):
        W, b = torch.as_tensor(params[2 * l]).to(torch.float64), torch.as_tensor(params[2 * l + 1]).to(torch.float64)
        z = F.linear(h, W, b)
        bound = (F.linear(h.abs(), W.abs()) + b.abs()) * ((W.shape[1] + 1) * 6e-8)
        out.append((z.abs() / bound).numpy())
        h = torch.relu(z)
    return out


def margin(params, x):
    """(N,) float64: the smallest |z| / ((n_in + 1) 6e-8 (|W||h| + |b|)) over the 512 hidden pre-activations of each point (render64.relu_margin's
    idea).  Below about 1 an fp32 evaluation may take the other side of a ReLU kink than float64."""
    return np.minimum.reduce([m.min(1) for m in unit_margins(params, x)])


def _point_grads(params64, xi, gi, flip=None):
    """the ten float64 gradients of one point, with the gate `flip` = (layer, unit) taking the other side than the float64 pre-activation says"""
    ps = [t.clone().requires_grad_(True) for t in params64]
    h = torch.as_tensor(xi).to(torch.float64)
    for l in range(4):
        z = F.linear(h, ps[2 * l], ps[2 * l + 1])
        gate = (z > 0).to(torch.float64).detach()
        if flip is not None and flip[0] == l:
            gate[0, flip[1]] = 1.0 - gate[0, flip[1]]
        h = z * gate
    m = torch.softmax(F.linear(h, ps[8], ps[9]), -1)
    return [t.numpy() for t in torch.autograd.grad((m * torch.as_tensor(gi).to(torch.float64)).sum(), ps)]


def gate_flips(params, x, g, limit=1.0):
    """[((point, layer, unit, unit margin), {gradient key: change})]: for every hidden unit within `limit` fp32 rounding bounds of its kink, what the
    ten gradients gain when that one gate takes the other side.  The mask does not move: the unit's value is zero to rounding on either side."""
    P = [torch.as_tensor(a).to(torch.float64) for a in params]
    out = []
    for l, um in enumerate(unit_margins(params, x)):
        for i, j in np.argwhere(um < limit):
            a, f = _point_grads(P, x[i:i + 1], g[i:i + 1]), _point_grads(P, x[i:i + 1], g[i:i + 1], (l, int(j)))
            out.append(((int(i), l, int(j), float(um[i, j])), {k: fk - ak for k, fk, ak in zip(GRAD_KEYS, f, a)}))
    return out


def admit_flips(got, ref, flips):
    """An fp32 evaluation may take either side of a gate that `gate_flips` lists, and each choice is a correct fp32 MaskField; the float64 yardstick
    takes one.  Returns (ref', taken): ref plus the changes of the listed gates that `got` took the other way - matching pursuit on the peak-scaled
    residual: the gate whose change explains the residual best is taken while its least-squares coefficient lies within 1 +- 0.25.  What the caller
    asserts is got against ref' under the UNCHANGED bound; the only freedom this adds is one bit per listed gate."""
    scale = {k: float(np.abs(ref[k]).max()) or 1.0 for k in GRAD_KEYS}
    vec = lambda d: np.concatenate([(np.asarray(d[k], np.float64) / scale[k]).ravel() for k in GRAD_KEYS])
    r = vec({k: np.asarray(got[k], np.float64) - ref[k] for k in GRAD_KEYS})
    vs = [vec(d) for _, d in flips]
    left, taken = set(range(len(flips))), []
    while left:
        best, cbest = None, 0.75
        for n in left:
            vv = float(vs[n] @ vs[n])
            c = float(r @ vs[n]) / vv if vv > 1e-24 else 0.0
            if abs(c - 1.0) < abs(cbest - 1.0):
                best, cbest = n, c
        if best is None:
            break
        r = r - vs[best]
        left.discard(best)
        taken.append(flips[best][0])
    out = {k: np.asarray(ref[k], np.float64).copy() for k in ref}
    for n, (tag, d) in enumerate(flips):
        if tag in taken:
            for k in GRAD_KEYS:
                out[k] = out[k] + d[k]
    return out, taken


def points(N, K, seed):
    """x (N, 3) uniform in [-1, 1]^3 and g (N, K) standard normal, fp32.  N <= 129: points with margin < KINK_MARGIN are redrawn.  (The hidden layers
    are the same for every K, so x depends on N and seed alone.)"""
    rng = np.random.default_rng(seed)
    x = (rng.random((N, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    if N <= 129:
        trunk = params_for(1)
        for _ in range(64):
            bad = np.nonzero(margin(trunk, x) < KINK_MARGIN)[0]
            if not len(bad):
                break
            x[bad] = rng.random((len(bad), 3), dtype=np.float32) * 2 - 1
        else:
            raise RuntimeError("points(): no kink-free draw")
    g = rng.standard_normal((N, K)).astype(np.float32)
    return x, g


def err(a, b):
    """max(maxrel, rel_l2) of conftest: the gradient metric"""
    return max(maxrel(a, b), rel_l2(a, b))


def case(K, N, steep=False):
    """(params, x, g) of a cell of MATRIX: what the GPU test uploads"""
    x, g = points(N, K, 7 * N + K)
    return params_for(K, steep), x, g


_yard = {}


def yardstick(K, N, steep=False, device="cpu"):
    """(y64, y32, bound) of a cell, computed once: the float64 yardstick, its float32 evaluation (always on the CPU) and bounds(y32, y64)"""
    key = (K, N, steep)
    if key not in _yard:
        p, x, g = case(K, N, steep)
        y64, y32 = mask64(p, x, g, device=device), mask64(p, x, g, dtype=torch.float32)
        _yard[key] = (y64, y32, bounds(y32, y64))
    return _yard[key]


def d32(y32, y64):
    """{mask: max abs, gradient key: max(maxrel, rel_l2)}: the float32 evaluation's distance from the yardstick"""
    out = {"mask": float(np.abs(y32["mask"].astype(np.float64) - y64["mask"]).max())}
    for k in GRAD_KEYS:
        if k in y64:
            out[k] = err(y32[k], y64[k])
    return out


def bounds(y32, y64):
    d = d32(y32, y64)
    return {k: max(3 * v, MASK_FLOOR if k == "mask" else FLOOR_G) for k, v in d.items()}


def group(K, N, steep=False):
    """the row of the figures table a cell belongs to"""
    kg = "steep" if steep else "K1-8" if K <= 8 else "K9-16" if K <= 16 else "K17-32"
    return kg, "N<=129" if N <= 129 else "N>129"
