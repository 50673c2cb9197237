"""Float64 yardstick of the distortion loss on ray weights (csrc/raydist.hip, nvfi_ray_distortion).

The kernel works on sample INDICES: D_r = delta [sum_ij w_i w_j |i - j| + 1/3 sum_i w_i^2] with delta = step / (far - near).  The yardstick
does not: it builds every sample's interval from the ray's geometry - z_j = t_min + step (j + u), the interval [z_j, z_j + step] mapped to
normalised distance s = (z - near) / (far - near) - and evaluates Mip-NeRF 360's loss for piecewise-constant intervals as written,

    D_r = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i          (m: interval midpoints, d: interval widths)

as a direct O(S^2) double sum in torch with autograd for the gradient, so the identity the kernel relies on (midpoints differ by exactly
(j - i) delta, jitter and t_min cancel) is itself under test.  dtype=torch.float32 gives the plain-fp32 floor of the same sums."""
import numpy as np
import torch

NEAR, FAR = 2.0, 6.0
CASES = ("spike", "two_surfaces", "fog", "zeros", "opaque")
PERIOD = 13          # a synthetic case has at most this many distinct rays: ray r repeats ray r % PERIOD, the yardstick runs once per distinct ray


def geometry(R, S, seed):
    """t_min (R,), u (R,), step of a case: float64, the samples stay inside [NEAR, FAR].  PERIOD values are drawn whatever R is: the first
    rows of a longer case are the shorter case"""
    rng = np.random.default_rng(1000 + seed)
    n = PERIOD
    step = (FAR - NEAR) * 0.85 / (S + 1)
    t_min = np.resize(NEAR + rng.uniform(0.0, 0.1 * (FAR - NEAR), n), R)
    u = np.resize(rng.uniform(0.0, 1.0, n), R)
    return t_min, u, step


def delta_of(step, near=NEAR, far=FAR):
    return step / (far - near)


def _weights_from_alpha(alpha):
    """w = alpha * T, T the exclusive cumulative product of (1 - alpha); the last sample keeps its alpha"""
    T = np.cumprod(np.concatenate([np.ones((alpha.shape[0], 1)), 1.0 - alpha[:, :-1]], axis=1), axis=1)
    return (alpha * T).astype(np.float32)


def named_case(name, R, S, seed):
    """(R, S) float32 weights of a seeded synthetic case; rays repeat with period PERIOD.  The PERIOD distinct rays are drawn whatever R is,
    so named_case(name, R, S, seed) is named_case(name, R2, S, seed)[:R] for every R2 >= R: a check made on five rays holds for the first
    five rays of the 257 the GPU tests upload.
    spike         one non-zero weight per ray (ray 0: the last sample, ray 1: the first, ray 2: sample min(64, S - 1))
    two_surfaces  a one-sample surface (alpha ~ 0.5; ray 0: at S // 2, the others up to three samples behind it, none in front: at S = 129 no
                  ray has it on sample 63, so swapping samples 63 / 64 moves every ray it touches the same way) and a soft one of optical depth ~1 behind it over a thin noisy background:
                  bimodal, and some weight reaches the last sample
    fog           many small weights (alpha ~ 3 / S with 50 % noise)
    zeros         two_surfaces with every ray r % 3 == 1 all zero
    opaque        a hard surface: the weights sum to 1 to rounding"""
    rng = np.random.default_rng(seed)
    n = PERIOD
    j = np.arange(S)[None, :]
    if name == "spike":
        w = np.zeros((n, S), np.float32)
        pos = rng.integers(0, S, n)
        pos[0], pos[1], pos[2] = S - 1, 0, min(64, S - 1)
        w[np.arange(n), pos] = rng.uniform(0.2, 1.0, n).astype(np.float32)
    elif name in ("two_surfaces", "zeros"):
        k1 = np.clip(S // 2 + rng.integers(0, 4, n), 0, S - 1)
        k1[0] = S // 2
        c2 = 0.8 * S + rng.uniform(-0.05, 0.05, n) * S
        alpha = 0.02 * rng.uniform(0.5, 1.5, (n, S)) * min(1.0, 64.0 / S)
        alpha += min(0.3, 6.4 / S) * np.exp(-0.5 * ((j - c2[:, None]) / max(S / 16.0, 0.5)) ** 2)
        alpha[np.arange(n), k1] = rng.uniform(0.4, 0.6, n)
        w = _weights_from_alpha(np.clip(alpha, 0.0, 1.0))
        if name == "zeros":
            w[1::3] = 0.0
    elif name == "fog":
        w = _weights_from_alpha(np.clip(3.0 / S * rng.uniform(0.5, 1.5, (n, S)), 0.0, 1.0))
    elif name == "opaque":
        k = rng.integers(0, S, n)
        alpha = np.where(j >= k[:, None], 0.9, 0.01 * rng.uniform(0.0, 1.0, (n, S)))
        alpha[:, -1] = 1.0
        w = _weights_from_alpha(alpha)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.resize(w, (R, S)))


def golden_map(gold, kind):
    """a real weight map of the committed hotpath fixture (a training render of golden field `kind` at a non-keyframe time) with
    delta = 1 / S: weights (R, S), t_min, u, step.  The jitter is the render's own."""
    w = np.ascontiguousarray(gold[f"{kind}:train_nonkey:weight"], np.float32)
    R, S = w.shape
    u = np.asarray(gold[f"{kind}:train_nonkey:u"], np.float64).reshape(-1)
    u = u if u.size == R else np.resize(u, R)
    return w, np.full(R, NEAR + 0.05), u, (FAR - NEAR) / S


SMALL = ((5, 1), (5, 2), (5, 65), (5, 129))      # (R, S) of the cases whose float64 results the fixture stores
FLOOR_EXTRA = ((5, 1024),)                        # measured for the floors only


def floor_inputs(gold):
    """every input the fp32 floors are measured on: (label, weights, t_min, u, step)"""
    for case in CASES:
        for (R, S) in SMALL + FLOOR_EXTRA:
            seed = CASES.index(case) * 100 + S
            t_min, u, step = geometry(R, S, seed)
            yield f"{case}:{R}x{S}", named_case(case, R, S, seed), t_min, u, step
    for kind in ("A", "B"):
        yield (f"map{kind}",) + golden_map(gold, kind)


def measure_floors(gold):
    """worst error of the float32 run of this yardstick against its float64 run: {loss, grad, per_ray}"""
    worst = {"loss": 0.0, "grad": 0.0, "per_ray": 0.0}
    for label, w, t_min, u, step in floor_inputs(gold):
        y, y32 = distortion(w, t_min, step, u), distortion(w, t_min, step, u, dtype=torch.float32)
        if y["loss"] == 0.0:
            continue
        e = errors(y32["loss"], y32["grad"], y32["per_ray"], y)
        for k, v in zip(("loss", "grad", "per_ray"), e):
            worst[k] = max(worst[k], v)
    return worst


def rays(weights, t_min, step, u, near=NEAR, far=FAR, dtype=torch.float64, chunk=8):
    """D_r (R,) and dD_r / dw (R, S) of every ray, numpy arrays of `dtype`: the direct double sum over explicit midpoints and widths,
    gradient by autograd"""
    wn = np.asarray(weights)
    R, S = wn.shape
    D, G = np.empty(R, np.float64), np.empty((R, S), np.float64)
    jj = torch.arange(S, dtype=torch.float64)
    for a in range(0, R, chunk):
        w = torch.tensor(wn[a:a + chunk], dtype=dtype, requires_grad=True)
        # the geometry is input data: midpoints and widths are formed in float64 whatever `dtype` is (in fp32 the difference of two midpoints
        # near 0.5 that lie 1e-3 apart would lose four digits, a floor of the geometry and not of the sums); the sums run in `dtype`
        tm = torch.tensor(np.asarray(t_min, np.float64)[a:a + chunk])[:, None]
        uu = torch.tensor(np.asarray(u, np.float64)[a:a + chunk])[:, None]
        z = tm + float(step) * (jj[None, :] + uu)
        lo, hi = (z - float(near)) / (float(far) - float(near)), (z + float(step) - float(near)) / (float(far) - float(near))
        mid, width = 0.5 * (lo + hi), (hi - lo).to(dtype)
        dist = (mid[:, :, None] - mid[:, None, :]).abs().to(dtype)             # (r, S, S): every pair of midpoints
        pair = (w[:, :, None] * w[:, None, :] * dist).sum(dim=(1, 2))
        d = pair + (w * w * width).sum(dim=1) / 3.0
        d.sum().backward()
        D[a:a + chunk] = d.detach().double().numpy()
        G[a:a + chunk] = w.grad.double().numpy()
    return D, G


def assemble(D, G, R=None, dtype=np.float64):
    """loss, per_ray, grad of the first R rays from rays(): loss = mean D_r, grad = dD_r/dw / R"""
    R = len(D) if R is None else R
    D, G = np.asarray(D[:R], dtype), np.asarray(G[:R], dtype)
    return {"loss": float(D.mean(dtype=dtype)) if R else 0.0, "per_ray": D.astype(np.float64), "grad": (G / dtype(max(R, 1))).astype(np.float64)}


def distortion(weights, t_min, step, u, near=NEAR, far=FAR, dtype=torch.float64):
    return assemble(*rays(weights, t_min, step, u, near, far, dtype), dtype=np.float64 if dtype == torch.float64 else np.float32)


def tiled(weights, t_min, step, u, R, near=NEAR, far=FAR, dtype=torch.float64):
    """distortion() of an R-ray case whose rays repeat with period PERIOD: the distinct rays are evaluated once"""
    n = min(R, PERIOD)
    D, G = rays(weights[:n], t_min[:n], step, u[:n], near, far, dtype)
    return np.resize(D, R), np.resize(G, (R, weights.shape[1]))


def index_form(weights, delta):
    """the form the kernel computes, in float64 numpy: loss, per_ray, and the closed-form gradient (delta / R) [2 (A + B) + 2/3 w]"""
    w = np.asarray(weights, np.float64)
    R, S = w.shape
    k = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :]).astype(np.float64)
    AB = w @ k                                                                  # A_i + B_i = sum_j |i - j| w_j
    per_ray = delta * ((w * AB).sum(1) + (w * w).sum(1) / 3.0)
    return {"loss": float(per_ray.mean()) if R else 0.0, "per_ray": per_ray, "grad": delta / max(R, 1) * (2.0 * AB + 2.0 / 3.0 * w)}


def _rel(a, b):
    """conftest.relerr's metric without its book-keeping: the larger of the max-norm and the L2 relative error"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if not b.size:
        return 0.0
    return float(max(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30), np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)))


def errors(loss, grad, per_ray, y):
    """(value error relative to |loss|, gradient error, per-ray error) against a yardstick result y; the tensor errors are
    max(max-norm, L2) relative errors, conftest.relerr's metric.  None for an output that was not produced."""
    e_l = None if loss is None else abs(float(loss) - y["loss"]) / (abs(y["loss"]) + 1e-300)
    e_g = None if grad is None else _rel(grad, y["grad"])
    e_p = None if per_ray is None else _rel(per_ray, y["per_ray"])
    return e_l, e_g, e_p


def bound(floor):
    """the project's bound per tensor: max(3 x the fp32 floor, 1e-5)"""
    return max(3.0 * float(floor), 1e-5)
