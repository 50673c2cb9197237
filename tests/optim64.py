"""Float64 yardstick of the part of a training iteration that is neither a render nor a loss term of its own: the plane regularisers
(density_L1 / TV_loss_density / TV_loss_app of the reference's models/tensorf_keyframe.py:188-231 with utils/tensorf_utils.py:139-158 TVLoss;
nvfi_plane_regs, csrc/regs.hip), the Adam update (the recurrence in the header of csrc/optim.hip; nvfi_adam_step) and the photometric MSE
(F.mse_loss; nvfi_mse).  Plain numpy, written from the mathematics.  tests/test_optim64_golden.py pins it to the reference's goldens and to torch
in float64; tests/test_gpu_optim64.py holds the device to it.

Every function takes `dtype`.  float64 is the reference.  float32 evaluates the same statements in float32: its distance from the float64
evaluation is the rounding a correct fp32 implementation may show, which is what the GPU tests derive their bounds from.

`mutate` (regs, mse) and plain argument changes (adam) give the deliberately wrong variants that the GPU tests use to show that their bounds
can see a subtly wrong kernel; they are never a reference."""
import numpy as np

SPACE_MODES = ((0, 1), (0, 2), (1, 2))      # plane i spans grid axes (W, H) = matModeSpace[i]; its time plane spans (matModeTime[i][0], K)
TIME_AXIS = (2, 1, 0)


def _tv(x, t, dt, skip_last_row=False, no_t3=False):
    """TVLoss(x, t) * 1e-2 of a (1, C, H, W) plane -> value, gradient"""
    _, c, h, w = x.shape
    dh = x[:, :, 1:, :] - x[:, :, :-1, :]
    dw = x[:, :, :, 1:] - x[:, :, :, :-1]
    if skip_last_row:
        dh = dh.copy()
        dh[:, :, -1, :] = 0
    hm = dt(3.0 if (t and not no_t3) else 1.0)
    sh = dt(2e-2) * hm / dt(c * (h - 1) * w)
    sw = dt(2e-2) / dt(c * h * (w - 1))
    val = sh * (dh * dh).sum(dtype=dt) + sw * (dw * dw).sum(dtype=dt)
    g = np.zeros_like(x)
    g[:, :, 1:, :] += dt(2) * sh * dh
    g[:, :, :-1, :] -= dt(2) * sh * dh
    g[:, :, :, 1:] += dt(2) * sw * dw
    g[:, :, :, :-1] -= dt(2) * sw * dw
    return val, g


def regs(planes, K, w3, dtype=np.float64, g0=None, mutate=None):
    """planes: the nine regularised planes dps[0..2], dpt[0..2], aps[0..2] as logical NCHW fp32 arrays; K: number of key frames; w3: the weights of
    (L1, TV density, TV app).
      L1  = sum_i mean|dps_i| + mean|1 - dpt_i|                 (sign(0) = 0)
      TVd = sum_i TV(dps_i) + TV_t(dpt_i)  [time planes only for K > 1],  TVa = sum_i TV(aps_i)
      TV(x) = 2 (h_tv / count_h + w_tv / count_w) * 1e-2,  h_tv = sum (x[y+1] - x[y])^2 (x 3 for a time plane: its rows are key frames), w_tv alike
    -> (L1, TVd, TVa), [g_0..g_8]: the gradients of w3 . (L1, TVd, TVa); with g0 (nine arrays) the result of ACCUMULATING them into g0 in `dtype`
    (what a gradient pass leaves in a .grad that was not empty; in float32 this includes the rounding of that addition).
    mutate: None | "last_row" (aps[0] without the vertical difference into its last row) | "no_t3" (time planes without the factor 3) |
            "last4" (dps[0] without the last four channels of its last texel: no L1 term, no gradient there)"""
    dt = np.dtype(dtype).type
    ps = [np.asarray(p, np.float32).astype(dtype) for p in planes]
    w = [dt(np.float32(x)) for x in w3]          # the C ABI and the device weights carry them as fp32
    L1, TVd, TVa = dt(0), dt(0), dt(0)
    out = []
    for k, x in enumerate(ps):
        g = np.zeros_like(x)
        kind, i = divmod(k, 3)                   # 0 density space, 1 density time, 2 appearance space
        n = dt(x.size)
        if kind == 0:
            a, s = np.abs(x), np.sign(x)
            if mutate == "last4" and i == 0:
                a, s = a.copy(), s.copy()
                a[0, -4:, -1, -1] = 0
                s[0, -4:, -1, -1] = 0
            L1 = L1 + a.sum(dtype=dt) / n
            g += (w[0] / n) * s
        elif kind == 1:
            u = dt(1) - x
            L1 = L1 + np.abs(u).sum(dtype=dt) / n
            g -= (w[0] / n) * np.sign(u)
        if kind != 1 or K > 1:
            v, gt = _tv(x, kind == 1, dt, skip_last_row=(mutate == "last_row" and k == 6), no_t3=(mutate == "no_t3"))
            if kind == 2:
                TVa = TVa + v
                g += w[2] * gt
            else:
                TVd = TVd + v
                g += w[1] * gt
        if mutate == "last4" and k == 0:
            g[0, -4:, -1, -1] = 0
        if g0 is not None:
            g = np.asarray(g0[k], np.float32).astype(dtype) + g
        out.append(g)
    return (L1, TVd, TVa), out


def adam(p, g_seq, lr_seq, b1, b2, eps, m0=None, v0=None, t0=0, dtype=np.float64):
    """torch.optim.Adam without amsgrad / weight decay, step by step (step t0+1, t0+2, ... with the gradients g_seq and learning rates lr_seq):
        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    b1, b2, eps and lr are first rounded to fp32 (the C ABI receives floats); the bias corrections are formed in double in every dtype (the host
    does that) and then carried in `dtype`.  p, m0, v0: fp32 arrays (m0, v0 default zeros) -> p, m, v in `dtype`"""
    dt = np.dtype(dtype).type
    b1f, b2f, epsf = (float(np.float32(x)) for x in (b1, b2, eps))
    p = np.asarray(p, np.float32).astype(dtype)
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float32).astype(dtype)
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float32).astype(dtype)
    cb1, cb2, ce = dt(b1f), dt(b2f), dt(epsf)
    t = int(t0)
    for g, lr in zip(g_seq, lr_seq):
        t += 1
        g = np.asarray(g, np.float32).astype(dtype)
        bc1, bc2 = 1.0 - b1f ** float(t), 1.0 - b2f ** float(t)
        step_size = dt(float(np.float32(lr)) / bc1)
        inv_sqrt_bc2 = dt(1.0 / np.sqrt(bc2))
        m = cb1 * m + (dt(1) - cb1) * g
        v = cb2 * v + (dt(1) - cb2) * g * g
        p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + ce)
    return p, m, v


def mse(x, y, dtype=np.float64, mutate=None):
    """mean((x - y)^2) and its gradient 2 (x - y) / n w.r.t. x.  mutate: None | "n-1" (divides by n - 1)"""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dtype)
    y = np.asarray(y, np.float32).astype(dtype)
    n = dt(x.size - (1 if mutate == "n-1" else 0))
    d = x - y
    return (d * d).sum(dtype=dt) / n, dt(2) * d / n


def err(a, b):
    """the suite's metric: max(max-norm relative error, relative L2 error); the relative error for a scalar"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if b.ndim == 0 or b.size == 1:
        a, b = float(a.reshape(-1)[0]), float(b.reshape(-1)[0])
        return abs(a - b) / abs(b) if b != 0 else abs(a)
    num = np.abs(a - b)
    return float(max(num.max() / (np.abs(b).max() + 1e-300), np.linalg.norm(num.ravel()) / (np.linalg.norm(b.ravel()) + 1e-300)))


def ulp_floor(ref, n_ulp=4.0):
    """n_ulp fp32 spacings at the quantity's peak, relative to that peak: the smallest distance from a float64 value that a result STORED in fp32
    can be asked to keep (a correctly rounded fp32 result is already up to half a spacing away)"""
    peak = float(np.max(np.abs(np.asarray(ref, np.float64)))) if np.size(ref) else 0.0
    if peak == 0.0:
        return 0.0
    return n_ulp * float(np.spacing(np.float32(peak))) / peak


def bound(y32, y64, margin=4.0):
    """margin x the distance of the float32 evaluation from the float64 one, and never below `margin` fp32 spacings of the peak"""
    return max(margin * err(y32, y64), ulp_floor(y64, margin))
