"""Float64 restatement of the stand-alone point queries (include/nvfi_hip.h: nvfi_vel_eval, nvfi_integrate_pos, nvfi_density_at, nvfi_app_at,
nvfi_render_mlp, nvfi_sh_render): the yardstick of tests/test_point64_golden.py (against the reference's goldens in tests/golden/hotpath.npz) and of
tests/test_gpu_point64.py (against the device).  Composed from the pieces the other yardsticks already hold: pde64._mlp (the velocity nets),
render64._planes / _pe / Field (the planes, the encodings, the parameters), advect64.rk2_back's gate / rejection / near-face bookkeeping,
flow64._near_face, alpha64.floors.  The statements:

  vel64        VelBasis.forward (velocity_field.py:69-98): (v, a) = (B_v(x) w(x, t), B_a(x) a_w(x, t)); gated: VelocityAABB[Sur].forward, v inside
               the gate box and exact zeros outside.
  integrate64  integrate_pos (tensorf_keyframe.py:575-611) with PER-POINT t and base: while off = t - base != 0: dt = sign(off) min(|off|, dt_max),
               x <- x - dt v_g(x - dt/2 v_g(x, t_c), t_c - dt/2), off -= dt, t_c -= dt; with the surround box a step that leaves it is rejected.
  density64    compute_densityfeature + feature2density (tensorf_keyframe.py:233-272, 312-321): sum_c prod_i space_i time_i, softplus(. + shift).
  app64        compute_appfeature + renderModule (tensorf_keyframe.py:274-310, tensorf_base.py:88-98): planes -> basis_mat -> MLPRender_PE or SHRender.
  mlp64        renderModule on the caller's features.
  sh64         SHRender (tensorf_model_utils.py:292-296): relu(sum_k SH_k(view) feat[9 c + k] + 0.5), degree 2.

As in render64 / alpha64, what the reference holds in fp32 before it touches the field stays fp32-rounded and is then promoted (the points, the views,
the features, the times); every discrete decision (gate, rejection, `unfinished`) is taken on fp32 values; the time recurrence of integrate_pos (off,
dt, t_curr, t_mid) runs per point in fp32 exactly as the reference's tensors and the device's registers run it, dt_max being the fp32 rounding of
0.5 tmax / (K - 1); it ends exactly, no snapping.  Everything else runs in `dtype`; dtype = float32 is "a plain fp32 implementation" of the same
statement, whose distance from the float64 run is the floor every bound below is derived from.

Each call has ONE deliberately wrong variant (`wrong=True`), computed here only; the bounds must see it (both test files assert that):
  integrate64: the midpoint evaluated at t_curr instead of t_curr - dt/2;  vel64: the acceleration formed with the velocity basis;
  density64: the time row index scaled by K / 2 instead of (K - 1) / 2;  app64 / mlp64: the view encoding's highest frequency dropped
  (MLP_PE; an SH field takes sh64's);  sh64: b[6] with zz - xx - yy instead of 2 zz - xx - yy."""
import numpy as np
import torch
import torch.nn.functional as F

import advect64
import alpha64
import flow64
import pde64
import render64 as r64

A_NAMES = pde64.NAMES[12:]
SIZES = alpha64.SIZES
DEEP_MAX_N = alpha64.MULTI_STEP_MAX_N       # the deep time case (`forward`) runs up to here
SWITCH_N = 32 * 4096                        # the last size on the four-wave x6 kernel; + 1 is the first on the one-wave-per-tile kernel
KINDS = ("A", "B", "D")                     # D: field A's geometry with SH shading (tests/golden/r2.npz)
MAX_STEPS = 4096                            # the library's cap for per-point times (max_steps of the kernels)


def field_of(sd, meta, sh=False):
    """render64.Field plus the a-net's parameters (a32) and the shading flag; an SH field has no render MLP: placeholders stand in for it"""
    sd = {(k[5:] if k.startswith("nvfi.") else k): np.asarray(v) for k, v in sd.items()}
    if sh:
        for n in r64.MLP_NAMES:
            sd.setdefault(n, np.zeros(1, np.float32))
    f = r64.Field(sd, meta)
    f.a32 = {k: torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)) for k in A_NAMES}
    f.sh = bool(sh)
    return f


def _t32(a, cols):
    """the fp32 rounding of an input as a fresh CPU tensor (N, cols), or (N,) with cols = 0: the caller's array is never aliased"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = np.array(a, dtype=np.float32, copy=True)
    return torch.from_numpy(a.reshape(-1, cols) if cols else a.reshape(-1))


def _params(field, names, dtype, device):
    src = dict(field.p32)
    src.update(getattr(field, "a32", {}))
    return {k: src[k].to(device=device, dtype=dtype) for k in names}


def _linear_chain(h, W, b):
    """fp32 Linear as the textbook dot product: acc = b, then acc = fl32(acc + h_k W_jk) for k = 0, 1, ... - one rounding per term (the product of
    two fp32 numbers is exact in float64), a chain of K sequential roundings per output"""
    Wt = W.t().contiguous().double()
    out = []
    for h1 in h.split(1024):           # (row blocks that stay in cache)
        acc, hd = b.expand(h1.shape[0], -1).clone(), h1.double()
        tmp = torch.empty(h1.shape[0], W.shape[0], dtype=torch.float64, device=h.device)
        for k in range(W.shape[1]):
            torch.addcmul(acc.double(), hd[:, k:k + 1], Wt[k], out=tmp)       # exact product, one rounding of the sum to float64 ...
            acc = tmp.float()                                                    # ... and to fp32 (the double rounding changes 1 sum in ~2^29)
        out.append(acc)
    return torch.cat(out)


def _mlp_chain(q, Ws, bs, act):
    """pde64._mlp in float32 with every layer summed sequentially (_linear_chain)"""
    assert q.dtype == torch.float32
    enc = [q]
    for k in range(3):
        enc += [torch.sin(q * 2.0 ** k), torch.cos(q * 2.0 ** k)]
    h = torch.cat(enc, -1)
    for i in range(6):
        h = _linear_chain(h, Ws[i], bs[i])
        if i < 5:
            h = act(h)
    return h


def _w_net(P, q, chain=False):
    return (_mlp_chain if chain else pde64._mlp)(q, [P[n] for n in r64.VEL_NAMES[0::2]], [P[n] for n in r64.VEL_NAMES[1::2]], F.silu)


def _v_of(w, x):
    px, py, pz = x[:, 0], x[:, 1], x[:, 2]
    return torch.stack([w[:, 0] - w[:, 4] * pz + w[:, 5] * py, w[:, 1] + w[:, 3] * pz - w[:, 5] * px, w[:, 2] - w[:, 3] * py + w[:, 4] * px], 1)


def _outside(p, lo, hi):
    p32 = p.to(torch.float32)
    return ((p32 < lo) | (p32 > hi)).any(-1)


def _near(p, field):
    return flow64._near_face(p.cpu(), field.lo, field.hi)


# ---------------------------------------------------------------------------------------------------------------- the six calls
def vel64(field, xt, gated, dtype=torch.float64, device="cpu", wrong=False, chain=False):
    """dict: u (N, 6) = (v, a), or (N, 3) gated with exact zeros outside the gate; edge (N,) bool: a coordinate within 4 fp32 ulp of a gate face;
    inside (N,) bool.  wrong: a = B_v(x) a_w instead of B_a(x) a_w.  chain (float32 only): every Linear layer summed sequentially, the OTHER plain
    fp32 order (see FLOOR below)"""
    q32 = _t32(xt, 4).to(device)
    q = q32.to(dtype)
    with torch.no_grad():
        P = _params(field, r64.VEL_NAMES + ([] if gated else A_NAMES), dtype, device)
        lo, hi = field.lo.to(device), field.hi.to(device)
        inside = ~_outside(q32[:, :3], lo, hi)
        v = _v_of(_w_net(P, q, chain), q[:, :3])
        if gated:
            u = torch.where(inside[:, None], v, torch.zeros_like(v))
        else:
            aw = (_mlp_chain if chain else pde64._mlp)(q, [P[n] for n in A_NAMES[0::2]], [P[n] for n in A_NAMES[1::2]], torch.relu)
            x, y, z = q[:, 0], q[:, 1], q[:, 2]
            a = _v_of(aw, q[:, :3]) if wrong else torch.stack([aw[:, 0] - (aw[:, 4] + aw[:, 5]) * x, aw[:, 1] - (aw[:, 3] + aw[:, 5]) * y,
                                                               aw[:, 2] - (aw[:, 3] + aw[:, 4]) * z], 1)
            u = torch.cat([v, a], 1)
    return dict(u=u.cpu().numpy(), edge=_near(q32[:, :3], field), inside=inside.cpu().numpy())


def integrate64(field, x, t, base, dtype=torch.float64, device="cpu", wrong=False, chain=False):
    """dict: xk (N, 3) numpy in `dtype`; steps (N,) int: the RK2 steps each point took; n_rejected: steps of points inside the surround box that left
    it (summed over points and steps); edge (N,) bool: a gate or rejection decision within 4 fp32 ulp of a face at some step; trace: per loop pass
    (t_curr, dt, t_mid, live) as fp32 / bool numpy arrays over all points.  wrong: the midpoint's time is t_curr.  chain (float32 only): the net's layers summed sequentially,
    as in vel64"""
    x32 = _t32(x, 3).to(device)
    N = x32.shape[0]
    tc = _t32(t, 0).to(device).clone()
    off = tc - _t32(base, 0).to(device)
    assert tc.shape[0] == N and off.shape[0] == N
    dt_max = torch.ones_like(tc) * (0.5 * field.tmax / (field.K - 1) if field.K > 1 else 1)
    lo, hi = field.lo.to(device), field.hi.to(device)
    pos = x32.to(dtype).clone()
    steps = torch.zeros(N, dtype=torch.int64, device=device)
    edge = np.zeros(N, bool)
    nrej, trace = 0, []
    with torch.no_grad():
        P = _params(field, r64.VEL_NAMES, dtype, device)

        def vel(p, tt):
            ins = ~_outside(p, lo, hi)
            v = _v_of(_w_net(P, torch.cat([p, tt.to(dtype)[:, None]], 1), chain), p)
            return torch.where(ins[:, None], v, torch.zeros_like(v))

        live = off.abs() > 0
        while bool(live.any()):
            if len(trace) >= MAX_STEPS:
                raise ValueError(f"a point needs more than {MAX_STEPS} RK2 steps")
            idx = live.nonzero()[:, 0]
            d = off[idx].sign() * torch.minimum(off[idx].abs(), dt_max[idx])
            tm = tc[idx] if wrong else tc[idx] - 0.5 * d
            cur = pos[idx]
            dd = d.to(dtype)[:, None]
            pm = cur - 0.5 * dd * vel(cur, tc[idx])
            xc = cur - dd * vel(pm, tm)
            e = _near(cur, field) | _near(pm, field)
            if field.sur:
                rej = _outside(xc, lo, hi)
                e |= _near(xc, field)
                nrej += int((rej & ~_outside(cur, lo, hi)).sum())          # (a point outside the gate never moves: not counted)
                xc = torch.where(rej[:, None], cur, xc)
            edge[idx.cpu().numpy()] |= e
            full = lambda v: torch.zeros(N, dtype=torch.float32, device=device).index_put((idx,), v).cpu().numpy()
            trace.append((tc.cpu().numpy().copy(), full(d), full(tc[idx] - 0.5 * d), live.cpu().numpy().copy()))
            pos[idx] = xc
            off[idx] = off[idx] - d
            tc[idx] = tc[idx] - d
            steps[idx] += 1
            live = off.abs() > 0
    return dict(xk=pos.cpu().numpy(), steps=steps.cpu().numpy(), n_rejected=nrej, edge=edge, trace=trace)


def density64(field, xyzt, dtype=torch.float64, device="cpu", wrong=False):
    """dict: feat (N,), sigma (N,) numpy in `dtype`.  wrong: the time row ((t' + 1) / 2) K instead of ((t' + 1) / 2) (K - 1)"""
    x4 = _t32(xyzt, 4).to(device=device, dtype=dtype)
    if wrong:
        x4 = torch.cat([x4[:, :3], (x4[:, 3:] + 1) * (field.K / (field.K - 1)) - 1], 1)
    with torch.no_grad():
        P = _params(field, [n for n in r64.PLANE_NAMES if n.startswith("density")], dtype, device)
        feat = r64._planes(P, "density", x4).sum(0)
        sigma = F.softplus(feat + field.shift)
    return dict(feat=feat.cpu().numpy(), sigma=sigma.cpu().numpy())


_sh = r64._sh          # the one statement of the degree-2 basis


def sh64(view, feat27, dtype=torch.float64, device="cpu", wrong=False):
    """(N, 3) numpy in `dtype`"""
    with torch.no_grad():
        return _sh(_t32(view, 3).to(device=device, dtype=dtype), _t32(feat27, 27).to(device=device, dtype=dtype), wrong).cpu().numpy()


def _render_module(field, P, x3, view, feat, wrong):
    if field.sh:
        return _sh(view, feat, wrong)
    pv = r64._pe(view, 6)
    if wrong:
        keep = torch.ones(36, dtype=pv.dtype, device=pv.device)
        keep[[5, 11, 17, 23, 29, 35]] = 0          # sin and cos of 2^5 view, per component (_pe: component-major, frequency-minor, sines first)
        pv = pv * keep
    h = torch.cat([feat, view, x3, r64._pe(x3, 6), pv], -1)
    for i in (0, 2, 4):
        z = F.linear(h, P[f"renderModule.mlp.{i}.weight"], P[f"renderModule.mlp.{i}.bias"])
        h = torch.relu(z) if i < 4 else torch.sigmoid(z)
    return h


def app64(field, xyzt, view, dtype=torch.float64, device="cpu", wrong=False):
    """dict: rgb (N, 3), feat (N, app_dim) numpy in `dtype`"""
    x4 = _t32(xyzt, 4).to(device=device, dtype=dtype)
    vw = _t32(view, 3).to(device=device, dtype=dtype)
    with torch.no_grad():
        P = _params(field, [n for n in r64.PLANE_NAMES if n.startswith("app")] + ["basis_mat.weight"] + ([] if field.sh else r64.MLP_NAMES), dtype, device)
        feat = F.linear(r64._planes(P, "app", x4).T, P["basis_mat.weight"])
        rgb = _render_module(field, P, x4[:, :3], vw, feat, wrong)
    return dict(rgb=rgb.cpu().numpy(), feat=feat.cpu().numpy())


def mlp64(field, xyz, view, feat, dtype=torch.float64, device="cpu", wrong=False):
    """(N, 3) numpy in `dtype`: renderModule(xyz, view, feat)"""
    with torch.no_grad():
        P = _params(field, [] if field.sh else r64.MLP_NAMES, dtype, device)
        n = 27 if field.sh else 32
        return _render_module(field, P, _t32(xyz, 3).to(device=device, dtype=dtype), _t32(view, 3).to(device=device, dtype=dtype),
                              _t32(feat, n).to(device=device, dtype=dtype), wrong).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- inputs of the test cases
N_FACE = 9
N_FAR = 16
SPECIAL_T = (-1.0, 1.0, 0.0, 1.0 / 3.0, -1.0 / 3.0, 0.99999, -0.99999, 0.5)       # tests/golden/make_golden.py: the time rows of the feature goldens


def _gate(field):
    lo, hi = field.lo.numpy().astype(np.float64), field.hi.numpy().astype(np.float64)
    return (lo + hi) / 2, (hi - lo) / 2


def case_points(field, N, kind):
    """deterministic fp32 inputs of a case of size N:
      "vel"      xt (N, 4): positions over 1.05 x the gate box, t in [0, 1]; from N = 31 on the first nine sit ON the gate box: two corners, the
                 centres of two faces, an edge, four points of faces (their gate decision compares equal numbers: no arithmetic, no freedom)
      "pos"      x (N, 3) over 1.05 x the gate box (on field B: 5 % beyond the surround box)
      "density"  xyzt (N, 4) over 1.15 x the unit box; the eight special time coordinates at the head (as many as fit), and the last
                 min(16, N - 8) points far outside: |coordinate| from 3 to 1e6, t' up to +-50, finite - every tap of some plane pair is padding
      "app"      (xyzt (N, 4) within 1.15 x the unit box with the special times at the head, view (N, 3) randn un-normalised, feat (N, app_dim) 0.3 randn)"""
    rng = np.random.default_rng({"vel": 1009, "pos": 2003, "density": 3001, "app": 4001}[kind] + N)
    if kind in ("vel", "pos"):
        c, h = _gate(field)
        x = (c + (rng.random((N, 3)) * 2 - 1) * 1.05 * h).astype(np.float32)
        if kind == "pos":
            return x
        tt = rng.random((N, 1)).astype(np.float32)
        if N >= 31:
            lo, hi, c32 = field.lo.numpy(), field.hi.numpy(), c.astype(np.float32)
            x[0], x[1] = lo, hi
            x[2] = (lo[0], c32[1], c32[2])
            x[3] = (c32[0], hi[1], c32[2])
            x[4] = (hi[0], hi[1], c32[2])
            x[5] = (x[5][0], x[5][1], lo[2])
            x[6] = (x[6][0], lo[1], x[6][2])
            x[7] = (hi[0], x[7][1], x[7][2])
            x[8] = (lo[0], hi[1], lo[2])
        return np.concatenate([x, tt], 1)
    q = (rng.random((N, 4)) * 2.3 - 1.15).astype(np.float32)
    k = min(len(SPECIAL_T), N)
    q[:k, 3] = np.asarray(SPECIAL_T[:k], np.float32)
    if kind == "density":
        nf = min(N_FAR, max(0, N - len(SPECIAL_T)))
        if nf:
            mag = np.logspace(np.log10(3.0), 6.0, N_FAR)[:nf, None] * np.where(rng.random((nf, 3)) < 0.5, -1.0, 1.0)
            far = np.concatenate([mag, np.linspace(-50.0, 50.0, N_FAR)[:nf, None]], 1).astype(np.float32)
            far[1::4, 3] = q[N - nf + 1:N:4, 3]        # every fourth keeps an in-range time: only its space taps are padding
            q[N - nf:] = far
        return q
    dim = 27 if field.sh else 32
    return q, rng.standard_normal((N, 3)).astype(np.float32), (0.3 * rng.standard_normal((N, dim))).astype(np.float32)


TIME_CASES = ("none", "mixed", "one_live", "forward", "tiny")
ONE_LIVE_STEPS = 8


def one_live_points(N):
    """the points of `one_live` that move: the last of the call and one in the middle of each 128-point workgroup"""
    return sorted({N - 1} | {i for i in range(64, N, 128)})


def time_cases(field, N, label):
    """(t, base) fp32 (N,) of a time case:
      none      t == base (a random time each): no point moves
      mixed     t uniform in [0, 1), base the snapped keyframe round(clamp(t / ts, 0, K - 1)) ts: 0 ... several steps, both signs, t > tmax extrapolates
      one_live  t == base except one_live_points(N), which take ONE_LIVE_STEPS steps (base 0, t = 7.5 dt_max)
      forward   t = 0, base per point in [0.5, 0.75): train_segm's argument order, negative steps; deep
      tiny      t = base (1 + 4e-6) with base the keyframe 1 + i mod (K - 1): one step of about 1e-8 ... 1e-6"""
    rng = np.random.default_rng({"none": 11, "mixed": 13, "one_live": 17, "forward": 19, "tiny": 23}[label] + N)
    ts = field.tmax / (field.K - 1)
    if label == "none":
        t = rng.random(N).astype(np.float32)
        return t, t.copy()
    if label == "mixed":
        t = torch.from_numpy(rng.random(N).astype(np.float32))
        base = torch.round((t / ts).clamp(0.0, field.K - 1)) * ts
        return t.numpy(), base.numpy()
    if label == "one_live":
        t = rng.random(N).astype(np.float32)
        base = t.copy()
        dtm = np.float32(0.5 * field.tmax / (field.K - 1))
        for i in one_live_points(N):
            t[i], base[i] = np.float32(7.5) * dtm, 0.0
        return t, base
    if label == "forward":
        return np.zeros(N, np.float32), (rng.random(N) * 0.25 + 0.5).astype(np.float32)
    if label == "tiny":
        base = np.array([np.float32((1 + i % (field.K - 1)) * ts) for i in range(N)], np.float32)
        return (base * np.float32(1 + 4e-6)).astype(np.float32), base
    raise KeyError(label)


def switch_inputs(field, N):
    """(x, t, base) of the `mixed` case either side of the kernel switch: the first N of the inputs of SWITCH_N + 1, so that the two calls share
    their first SWITCH_N points"""
    t, base = time_cases(field, SWITCH_N + 1, "mixed")
    return case_points(field, SWITCH_N + 1, "pos")[:N], t[:N], base[:N]


def case_sizes(label):
    return tuple(n for n in SIZES if n <= DEEP_MAX_N) if label == "forward" else SIZES


# ---------------------------------------------------------------------------------------------------------------- bounds
def bound(floor_abs, floor_rel, scale):
    """(rtol, atol) from a float32 floor (alpha64.floors): 3 x each, never under one fp32 ulp (of `scale` for the absolute part)"""
    return max(3 * floor_rel, advect64.ULP32), max(3 * floor_abs, advect64.ULP32 * scale)


def excess(got, ref, rtol, atol):
    """the largest |got - ref| - (rtol |ref| + atol); <= 0: every element is inside the bound"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) - rtol * np.abs(ref) - atol).max()) if ref.size else -float(atol)


# The float32 floors (abs, rel as alpha64.floors gives them: abs over the elements with |ref| <= 1e-2, rel over the rest) of each call, field and
# case of tests/test_gpu_point64.py: the float32 evaluation of the yardstick against its float64 evaluation, points near a gate face left out,
# worst over the case's sizes (alpha64.SIZES; `forward` up to 257; `mixed` also at 32 * 4096 and 32 * 4096 + 1), measured on the CPU (torch 2.10)
# and rounded up to two digits.  tests/test_point64_golden.py measures them again and fails when 3 x one of them leaves the bound below.
# Every call whose RESULT is the velocity net's output or is built from it - vel, vel_gated, integrate - takes the worse of TWO plain fp32
# evaluations: torch's (a blocked sum per output) and the textbook dot product summed term by term (_linear_chain: K = 128 sequential roundings per
# output, the order in which a matrix-pipe accumulator - or a C loop - adds).  The rounding error of a K-term fp32 sum depends on the order
# (Higham, Accuracy and Stability of Numerical Algorithms, ch. 4: ~K u sequentially, ~(K / b + b) u in blocks of b): a floor taken from the blocked
# order alone is that order's, not fp32's.  This changes what "a plain fp32 implementation" means for the floor, not the float64 yardstick; it was
# found by tests/test_gpu_point64.py (its docstring has the figures), and both evaluations run on the CPU.  The blocked order alone gives (A | B):
#   vel 9.9e-8, 4.0e-6 | 1.1e-7, 9.5e-7    vel_gated 9.9e-8, 1.2e-6 | 1.1e-7, 2.0e-6    mixed 1.5e-8, 4.7e-7 | 2.2e-8, 3.6e-7
#   one_live 1.7e-8, 9.6e-7 | 3.2e-9, 3.9e-7    forward 2.9e-8, 1.9e-6 | 8.5e-8, 3.9e-6    tiny: the same in both orders
# (the sequential order is measured at alpha64.SIZES, where both integrators run; the two sizes at the kernel switch add the blocked order only).
# The colours and features keep the blocked order's floor alone, the smaller of the two: no plane lookup has a long sum, and the render MLP's
# output passes a sigmoid; the device meets it.
# Fields: A (VelocityAABB, K = 4), B (VelocityAABBSur, K = 16), D (A's geometry, SH shading).  The SH colours carry the cancellation of
# relu(sum + 0.5) next to zero with |view|^2 up to ~10: their relative floor is the largest of the table.
FLOOR = {
    ("vel", "A", "all"): (4.3e-7, 1.8e-5), ("vel", "B", "all"): (3.7e-7, 1.1e-5),
    ("vel_gated", "A", "all"): (4.0e-7, 2.5e-5), ("vel_gated", "B", "all"): (3.7e-7, 1.1e-5),
    ("integrate", "A", "none"): (0.0, 0.0), ("integrate", "B", "none"): (0.0, 0.0),
    ("integrate", "A", "mixed"): (7.2e-8, 2.6e-6), ("integrate", "B", "mixed"): (3.6e-8, 6.1e-7),
    ("integrate", "A", "one_live"): (5.9e-8, 4.4e-6), ("integrate", "B", "one_live"): (1.3e-8, 6.1e-7),
    ("integrate", "A", "forward"): (2.1e-7, 6.4e-6), ("integrate", "B", "forward"): (8.5e-8, 5.7e-6),
    ("integrate", "A", "tiny"): (4.7e-10, 5.9e-8), ("integrate", "B", "tiny"): (4.7e-10, 5.9e-8),
    ("feat", "A", "all"): (2.1e-7, 1.1e-5), ("feat", "B", "all"): (2.2e-7, 8.5e-6),
    ("sigma", "A", "all"): (3.3e-8, 5.4e-6), ("sigma", "B", "all"): (2.7e-8, 7.6e-6),
    ("app", "A", "all"): (0.0, 1.5e-7), ("app", "B", "all"): (0.0, 1.4e-7), ("app", "D", "all"): (2.1e-6, 4.8e-5),
    ("mlp", "A", "all"): (0.0, 1.4e-7), ("mlp", "B", "all"): (0.0, 1.4e-7), ("mlp", "D", "all"): (2.2e-7, 6.6e-6),
    ("sh", "D", "all"): (2.2e-7, 6.6e-6),
}
# the scale whose fp32 ulp no atol goes under: positions, velocities and colours are of order 1 (features are larger: 1 is the stricter choice);
# sigma of these inputs stays under 0.3
SCALE = {"sigma": 0.25}
# The bounds the device is held to, |got - ref| <= rtol |ref| + atol: exactly 3 x the recorded floor, never under one fp32 ulp
POINT_RTOL = {k: bound(fa, fr, SCALE.get(k[0], 1.0))[0] for k, (fa, fr) in FLOOR.items()}
POINT_ATOL = {k: bound(fa, fr, SCALE.get(k[0], 1.0))[1] for k, (fa, fr) in FLOOR.items()}
