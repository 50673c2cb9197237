"""The timed training iteration - bench.Step and bench.GraphedStep, the drivers behind bench.py's headline number - against the float64 yardstick
of one iteration (tests/step64.py, pinned to the reference's own loop by tests/test_step64_golden.py), in every launch mode.

tests/step64_worker.py runs each mode in a process of its own: one set-up step, then three recorded iterations.  The comparison is teacher-forced:
for every iteration the yardstick starts from the device's OWN state before it (parameters, exp_avg, exp_avg_sq), the inputs it consumed (rays,
targets, jitter, times, collocation points), its own appearance masks and its own PDE kept set, and the iteration index - the schedule (loss weights,
learning rates, Adam's step count) is computed from that index inside the yardstick, never read from the driver.

Asserted per mode and iteration (_check):
  maps      both colour maps element-wise within MAP_RTOL x |ref| + helpers.FP32_FLOOR (MAP_RTOL = 5e-5 as in test_gpu_render64.py - the same kernels
            on rays of the same camera bundle; the float32 evaluation of the yardstick has to keep a third of it here, asserted)
  values    the returned loss (the MSE of the last render), last_lv and the three regulariser values within optim64.bound(float32, float64)
  counters  valid, in-gate and masked counts equal the yardstick's; the device's masks differ from the yardstick's own on at most 0.1 % of the masked
            samples, each within 2e-6 of the threshold; the PDE kept set against step64.kept64 by the same rule; last_pde_out[1] is the kept count
  gradient  recovered from the moments in float64, g_dev = (m_after - b1 m_before) / (1 - b1), against the yardstick's total gradient through
            assert_grad with max(maxrel, rel_l2) <= B[family]; v_after against b2 v_before + (1 - b2) g64^2 within 2 B[family] + the fp32 floor
  update    the last line of Adam from the device's own exp_avg / exp_avg_sq, every element, to five fp32 roundings and half a spacing of p; and
            on the distance moved, |dp_dev - dp_64| <= B_p x lr_t.  Exempt: an element with 0 < |g64| < B[family] x max|g64| of its tensor may take
            either sign at full step length and only has to stay within lr_t x 1.001 / (1 - b1); at most 2 % of a tensor of 64 or more elements may be
            exempt (a condition on the scene and seeds, asserted from the yardstick).  Where g64 is exactly zero and the element has no history,
            parameter and moments stay bit-equal
  buffers   the flat gradient buffer is all zero bits after the step; in shadow3 the field's own parameters are bit-unchanged
  schedule  param_groups[*]["lr"], L1w, tvd, tva, vw and Adam's step after the iteration equal the yardstick's for that index; in the record modes
            rec[2:6] and the Adam scalars rec[16:] equal the fp32 rounding of the yardstick's values, and rec[0:2] equals the host's fp32 times
Across modes: eager1, eager3, shadow3, record and replay draw bit-equal rays, targets, points, times and jitter (test_modes_see_the_same_draws).

Bounds are derived at run time from the yardstick; the two that are typed in (APP_TIME_B, the ceilings of OVER_CAP) are named below.  B[family] (density planes, appearance planes, render MLP + basis_mat, velocity nets) is, per mode and iteration, 3 x the
distance of step64(float32) from step64(float64) on that very case and mask - the float32 gradient recovered from ITS fp32 moments by the same
formula, so that the rounding of the recovery is part of the figure.  B_p is 3 x the largest |dp_32 - dp_64| / lr_t over the non-exempt elements.
The upper limits are the wrong variants of the yardstick (step64.VARIANTS): a bound sees a variant if the variant moves the observable by 3 x the
bound or more.  Every variant has to be seen by some asserted observable in some iteration of a mode, or be listed in BLIND for that mode kind,
which is then asserted to BE blind (test_every_wrong_variant_is_seen).

B[family] is the lower limit, 3 x the float32 figure.  The float32 run is plain fp32 down to its sums over the rays and points (render64 / pde64
add their chunks up in float32) and is taken in two orders on the device the references run on: chunks of 256 rays / 32 768 points and chunks of 32 /
4 096, eight times as many sequential additions; the figure is the larger of the two.  The upper limit - a third of the smallest move that a
wrong variant (d), (e), (f), (g) makes in the family - is measured and printed beside it.
The appearance branch (render MLP, basis_mat, appearance planes) has a floor under its B.  The kernels add one contribution per masked sample with
fp32 atomics, per 32-sample tile; torch's float32 sums are blocked, and neither chunk length brings them near a sequential sum of that length (the
figure stays at 9e-7 - 1.3e-6 down to chunks of 4 rays).  A sequential fp32 sum of N terms of one sign carries a relative error of u sqrt(N / 3):
a random walk of roundings u = 2^-24 on partial sums that grow linearly.  renderModule.mlp.4.bias shows that this is what separates the two: its
three elements are exactly such a sum, no ReLU decision touches it (render64's kink bracket, decisions taken one rounding bound either side,
moves it by 1e-9 and the hidden layers by 1e-3), and it sits at 3.0e-6 - 3.7e-6 on the device against 9.5e-7 in float32, with u sqrt(N / 3) =
9.2e-6 at the 72 000 masked samples of an iteration.  The floor is 3 u sqrt(N / 3) with N the yardstick's own masked count: 2.7e-5 - 2.8e-5 on the
two-render workload, 1.9e-5 - 2.0e-5 on the radiance-only one.  The exempt set and B_p are formed with 3 x the float32 figure alone.
One class has a bound of its own, APP_TIME_B = 1e-4 for app_plane_time.*: their gradients are 1e-10 and nearly cancel, so the sum is far from one
sign; in the third iteration the device is 2.5e-5 - 3.8e-5 of the peak off there (eager1, eager3, record) where the float32 runs sit at 2.4e-6.
tests/test_gpu_render64.py records 2.9e-5 (device) and 3.0e-5 (render64 in float32) for the appearance planes of this field at a non-keyframe time
and bounds them by 1e-4; that bound is taken over for these three tensors.

Measured on one MI355X (24 tests, 60 - 62 s, three runs with all 24 passing; the first case of a mode 5 - 10 s with its worker of 4 - 6 s, the
others 1 - 2 s; WORKER_LIMIT is 40 x that).  The GPU suite without this file takes 472 s in the same tree, 533 s with it.
  gradient, 3 x float32 / B / a third of the nearest variant / device (density, vel: B is 3 x float32)
    eager1 it1   density 3.0e-6 / 8.3e-3 / 8.1e-7   app 7.6e-6 / 2.8e-5 / 3.3e-1 / 5.0e-6   mlp 9.4e-6 / 2.8e-5 / - / 3.1e-6      vel 8.8e-6 / 6.5e-2 / 2.6e-7
    eager1 it2   density 4.1e-6 / 7.8e-3 / 1.1e-6   app 4.0e-5 / 4.0e-5 / 3.2e-1 / 2.9e-6   mlp 9.1e-6 / 2.8e-5 / 9.7e-2 / 3.0e-6 vel 9.6e-6 / 1.2e-1 / 4.5e-7
    eager1 it3   density 2.7e-6 / 7.9e-3 / 1.1e-6   app 7.4e-6 / 2.7e-5 / 2.5e-1 / 3.8e-5*  mlp 1.2e-5 / 2.7e-5 / 9.6e-2 / 9.5e-6 vel 1.2e-5 / 1.9e-1 / 6.9e-7
    eager3, record: as eager1 to two digits in every iteration (it3: app 3.8e-5*, mlp 9.4e-6 / 9.5e-6)
    shadow3 it1  density 2.7e-6 / 8.6e-3 / 8.5e-7   app 6.1e-4 / 6.1e-4 / 3.3e-1 / 2.6e-6   mlp 9.9e-5 / 9.9e-5 / - / 3.2e-6      vel 8.8e-6 / 3.8e-2 / 3.7e-7
    shadow3 it2  density 4.3e-6 / - / 1.4e-6        app 2.8e-3 / 2.8e-3 / - / 9.4e-4        mlp 2.9e-4 / 2.9e-4 / 3.4e-1 / 9.5e-5 vel 1.2e-5 / 3.0e-2 / 3.7e-7
    replay it2   density 3.5e-6 / 7.5e-3 / 1.2e-6   app 6.4e-5 / 6.4e-5 / 3.3e-1 / 2.1e-5   mlp 1.3e-5 / 2.8e-5 / - / 4.3e-6      vel 9.2e-6 / 1.2e-1 / 3.7e-7
    replay it4   density 2.9e-6 / 7.4e-3 / 9.8e-7   app 7.5e-6 / 2.7e-5 / 3.1e-1 / 2.5e-6   mlp 1.8e-5 / 2.7e-5 / 2.0e-1 / 5.9e-6 vel 5.6e-5 / 3.7e-1 / 7.7e-7
    cfg2_eager   density 3.8e-6 - 5.0e-6 / 1.4e-2 / 1.3e-6 - 1.6e-6   app 7.6e-6 - 9.9e-6 / 2.0e-5 / 2.5e-1 / 2.3e-6 - 3.3e-6   mlp 9.2e-6 - 1.1e-5 / 2.0e-5 / 9.1e-2 / 2.7e-6 - 3.3e-6
    cfg2_replay  density 2.7e-6 - 5.1e-6 / 1.4e-2 / 9.6e-7 - 1.5e-6   app 6.9e-6 - 7.6e-6 / 2.0e-5 / 2.5e-1 / 2.3e-6 - 2.6e-6   mlp 1.1e-5 - 1.4e-5 / 2.0e-5 / 9.9e-2 / 2.7e-6 - 4.7e-6
  (* app_plane_time.0 - .2, held to APP_TIME_B; the appearance space planes sit at 2.7e-6 there.  No variant moves the render MLP in a first
  iteration: (d) and (e) need a previous one.  In shadow3's second iteration the moments carry a long history against a small gradient: the
  recovery from fp32 moments costs the float32 runs and the device alike their digits, 9.4e-4 on both sides.)
  update, B_p / device (units of lr_t): eager1, eager3, record 3.0e-4 / 1.0e-4, 1.4e-4 / 4.6e-5, 1.2e-3 / 4.1e-4; shadow3 1.4e-2 / 9.6e-5, 1.5e-2 /
    4.8e-3, 1.6e-4 / 5.2e-5; replay 1.2e-3 / 4.0e-4, 8.7e-4 / 2.9e-4, 3.1e-3 / 4.1e-5; cfg2_eager 4.4e-4 / 1.4e-4, 1.2e-4 / 3.8e-5, 1.2e-4 / 4.0e-5;
    cfg2_replay 1.5e-4 / 5.0e-5, 1.2e-4 / 3.9e-5, 6.8e-5 / 2.3e-5.  The update from the device's own moments holds on every element.
  values: loss 2.1e-7 - 3.5e-7 (bound 1.1e-6 - 1.2e-6), L1 / TVd / TVa at most 8.6e-8 (bounds 2.4e-7 - 4.7e-7), last_lv at most 6.4e-8 (bound 2.4e-7 -
  4.6e-7); maps at most 5.5e-7 absolute.  Every mask was observable; the PDE kept set equals step64.kept64 except for one point of shadow3's third
  iteration, 1.4e-8 from the threshold.
  wrong variants: (d), (e), (f1), (f2), (g) move a gradient by 1e4 - 1e6 x its B and the update by 400 - 6000 x B_p; (a) the gradient by 10 - 42 x B
    (a_weight_net, which only the PDE term reaches) and the update by up to 7.6 x B_p; (c) the update by 24 - 1168 x B_p.  (b), the learning rate
    decayed before the step, moves the update by 0.3 B_p at most and leaves the same schedule behind: it is seen by the update from the device's
    own moments, which is formed with the yardstick's lr_t (7.7e-5 relative against a tolerance of 5e-7), and in the record modes by the
    scalars the device read (rec[2:6], rec[16:]; _record forms the variant's, and they differ from the right ones).  BLIND is empty.

The exempt share.  The 2 % cap is NOT met on this scene, whatever the seed; largest share per tensor over the 21 cases (OVER_CAP holds a ceiling
above each - the share plus half a per cent of the tensor, or four elements of a small one -, every tensor that is not listed keeps 2 %):
  density_plane_time.0 / .1 / .2  12.8 / 12.5 / 12.2 %, app_plane_time.0 / .1 / .2  14.7 / 14.6 / 14.2 % (shadow3, second iteration).  Of these
    12.2 / 12.5 / 11.8 % are rows beside a base keyframe row: the normalised keyframe time 2 k / 15 - 1 is exact in binary only for k = 0 and 15;
    elsewhere the fp32 row coordinate lies 3e-8 - 1e-6 beside its integer, the next row gets that weight and a gradient of 1e-7 of the peak - one
    or two of 16 rows in every iteration, for every seed whose renders are not all at t = 0 or t = 0.75.
  renderModule.mlp.0.weight 30.0 % (never under 27.8 %: the 32 appearance-feature columns of 110 see inputs of 1e-6), mlp.2.weight 12.5 %,
    mlp.2.bias 5.5 %, mlp.4.weight 7.0 % (shadow3, second iteration; 2.3 - 4 % elsewhere: dead hidden units).
  vel_net.a_weight_net.3.0 / 4.0 / 5.0 / 6.0.weight 4.3 / 4.9 / 5.4 / 4.6 % (replay, third iteration; 2.0 - 2.5 % elsewhere: units of the ReLU net
    that few kept points reach).  The shares are those of the velocity perturbation of tests/pde64_worker.py; another one was not tried.
  Under the cap: the six space planes (at most 0.73 %), basis_mat.weight (0.07 %), every bias but mlp.2.bias, weight_net (at most 1.8 %).
  The ceilings hold over all modes; the shares repeat to four digits from run to run (the device's state differs by the order of its atomics only).
An exempt element is not unchecked: its gradient is inside maxrel, its exp_avg_sq inside the v check, and its update has to be Adam's last line
applied to the device's own moments, to five fp32 roundings.

Two mutations of the library that change values only, each built apart and run once against this file and the older GPU suite (without
test_gpu_render64.py, test_gpu_pde64.py and the two packet-capture cases of test_gpu_graph.py, none of which launches Adam or the regularisers):
  (A) k_adam ignoring its zero_grad flag for the last tensor of the table: failed all 21 cases of test_iteration_matches_float64 - the flat buffer
      is not all zero bits in every one, and the gradient, exp_avg_sq and update of the table's last tensor (vel_net.a_weight_net.7.0.bias; on the
      radiance-only workload renderModule.mlp.4.bias) leave their bounds.  Of the older tests 12 failed: test_gpu_graph.py::
      test_adam_with_device_side_scalars_is_bit_identical, nine of test_gpu_optim64.py's Adam tests, test_gpu_parity.py::test_fused_adam_matches_torch
      and test_gpu_round5.py::test_round4_launch_chain_still_matches_goldens.  The kernel was not without a net; no older test saw it through
      bench.Step (test_gpu_graph's replay test, test_gpu_bench_outputs.py and test_gpu_training_loop.py's fused driver passed).
  (B) nvfi_plane_regs_dev taking the TV-appearance weight from the TV-density slot: NOT seen by this file - it cannot be seen through bench's
      drivers at all: tvd and tva both start at 1.0 and decay by the same factor, so rec[3] == rec[4] bit for bit in every iteration.  The older
      suite sees it in 17 tests that pass unequal weights (test_gpu_graph.py::test_device_side_weights_match_host_scalars, twelve of
      test_gpu_optim64.py, test_gpu_parity.py::test_plane_regularisers[A, B], test_round4_launch_chain_still_matches_goldens,
      test_three_training_iterations_match_the_reference[dropin-pure-autograd]).
No defect of the library, of optim.py, dist.py, the field's host path or bench.py was found.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, assert_grad, maxrel, outfrac, rel_l2

sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (before anything initialises the GPU, as tests/test_gpu_graph.py needs it)

import optim64  # noqa: E402
import step64 as s64  # noqa: E402
from helpers import FP32_FLOOR, field_state  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["eager1", "eager3", "shadow3", "record", "replay", "cfg2_eager", "cfg2_replay"]
RECORD_MODES = ("record", "replay", "cfg2_replay")
SAME_DRAWS = ["eager1", "eager3", "shadow3", "record", "replay"]
MAP_RTOL = 5e-5
EXEMPT_CAP = 0.02
WORKER_LIMIT = 240          # seconds; a worker takes 4 - 6 s on an MI355X (scene build and import included)
# (mode kind, variant) that no asserted observable of that kind of mode can see: asserted to be blind.  None: the eager modes hold no record of
# the scalars the device used, but the update from the device's own moments is formed with the yardstick's learning rate and bias corrections
BLIND = set()

# The appearance time planes: the bound that tests/test_gpu_render64.py derives for the appearance planes of the bench field at a non-keyframe time
# (B_R["head_nonkey"], 3 x the float32 figure 3.0e-5 of render64 there).  Their gradients are 1e-10 and nearly cancel; the float32 evaluations of
# THIS case happen to sit at 2.4e-6 in the third iteration, where a correct fp32 render is known to sit at 3e-5 (the docstring has the figures)
APP_TIME_B = 1e-4
# Tensors that cannot keep the 2 % cap on the scene this file has to use, whatever the seed, each with a ceiling just above the largest share measured
# in any mode and iteration (the docstring says why each is there).  A tensor that is not listed keeps the cap; a listed one keeps its ceiling and
# has to be over the cap somewhere, or the entry has outlived its reason.
OVER_CAP = {"density_plane_time.0": 0.133,
            "density_plane_time.1": 0.130,
            "density_plane_time.2": 0.127,
            "app_plane_time.0": 0.152,
            "app_plane_time.1": 0.152,
            "app_plane_time.2": 0.147,
            "renderModule.mlp.0.weight": 0.305,
            "renderModule.mlp.2.weight": 0.131,
            "vel_net.a_weight_net.3.0.weight": 0.048,
            "vel_net.a_weight_net.4.0.weight": 0.055,
            "vel_net.a_weight_net.5.0.weight": 0.060,
            "vel_net.a_weight_net.6.0.weight": 0.051,
            "renderModule.mlp.2.bias": 0.086,
            "renderModule.mlp.4.weight": 0.081}
_runs, _failed, _meta, _cache = {}, [], {}, {}
_T0 = time.time()


def _worker(mode):
    """one worker process per mode; after a failed one no further worker is started"""
    if mode in _runs:
        return _runs[mode]
    if _failed:
        pytest.fail(f"not run: the worker of {_failed[0]} failed")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"step64_{os.getpid()}_{mode}.npz")
    _failed.append(mode)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "step64_worker.py"), out, mode], capture_output=True, text=True,
                           timeout=WORKER_LIMIT)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"worker {mode} ran into its time limit:\n" + str(e.stdout)[-2000:] + str(e.stderr)[-3000:])
    if r.returncode != 0:
        pytest.fail(f"worker {mode} exited with {r.returncode}:\n" + r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    _runs[mode] = {k: z[k] for k in z.files}
    os.remove(out)
    _failed.remove(mode)
    print(r.stdout, flush=True)
    return _runs[mode]


def _device():
    import torch
    return "cuda" if torch.cuda.is_available() else "cpu"


def _scene(cfg2):
    """the configuration scalars and the tensors no optimiser group holds (the velocity nets of the radiance-only field): the scene rebuilt on the CPU"""
    if cfg2 not in _meta:
        import torch
        import step64_worker as W
        m = W.scene(torch.device("cpu"), cfg2)
        sd, meta = field_state(m)
        _meta[cfg2] = ({k: np.asarray(v) for k, v in sd.items()}, meta)
    return _meta[cfg2]


def _metric(a, b):
    return max(maxrel(a, b), rel_l2(a, b))


def _state(z, k, tag):
    names = [str(n) for n in z["names"]]
    return tuple({n: z[f"it{k}:{tag}:{x}:{n}"] for n in names} for x in "pmv")


def _case(mode, k):
    """the yardstick on iteration k of a mode: float64, float32 and every wrong variant, computed once"""
    if (mode, k) in _cache:
        return _cache[(mode, k)]
    import torch
    z = _worker(mode)
    cfg2 = bool(z["cfg2"])
    sd, meta = _scene(cfg2)
    it = int(z["it0"]) + k
    p, m, v = _state(z, k, "before")
    full = dict(sd)
    full.update(p)
    if mode == "shadow3":                    # the shadow step updates a copy; the iteration itself renders the FIELD's parameters
        full.update({n: z[f"it{k}:before:field:{n}"] for n in p})
    field, params_all = s64.make_field(full, meta)
    field.use_vel = not cfg2
    nb = 1 if cfg2 else 2
    batches = [dict(o=z[f"it{k}:o{b}"], d=z[f"it{k}:d{b}"], target=z[f"it{k}:tg{b}"], u=z[f"it{k}:u{b}"], t=float(z[f"it{k}:t"][b])) for b in range(nb)]
    masks = [z.get(f"it{k}:mask{b}") for b in range(nb)]
    dev = _device()
    pde, kept_own = None, None
    if not cfg2:
        s64.load(field, params_all)
        kept_own = s64.kept64(field, z[f"it{k}:pts"], z[f"it{k}:pt"], device=dev)
        pde = dict(points=z[f"it{k}:pts"], t=z[f"it{k}:pt"], kept=z[f"it{k}:kept"] if f"it{k}:kept" in z else kept_own[0])
    render_params = {n: params_all[n] for n in params_all}
    T = {dt: s64.terms(field, render_params, batches, pde, True, masks, dt, dev) for dt in (torch.float64, torch.float32)}
    # a second plain fp32 order of the same statement: short chunks, i.e. eight times as many sequential fp32 additions over the rays and points
    r32b = s64.combine(p, m, v, it, s64.terms(field, render_params, batches, pde, True, masks, torch.float32, dev, chunk=32, pde_chunk=4096), field.K,
                       torch.float32, reg_params=render_params)
    # the step is taken on the optimiser's own tensors (shadow3: the copies), the gradient comes from the field's
    ref = s64.combine(p, m, v, it, T[torch.float64], field.K, torch.float64, reg_params=render_params)
    r32 = s64.combine(p, m, v, it, T[torch.float32], field.K, torch.float32, reg_params=render_params)
    var = {}
    g_prev = None
    if k > 0:
        g_prev = _case(mode, k - 1)["ref"]["grads"]
    for name in s64.VARIANTS:
        if name in ("d", "e") and k == 0:
            continue
        if name in ("f1", "f2") and cfg2:
            continue
        if name == "e":
            prev = _case(mode, k - 1)["render_params"]
            Ts = s64.terms(field, prev, batches, pde, True, masks, torch.float64, dev)
            var[name] = s64.combine(p, m, v, it, Ts, field.K, torch.float64, reg_params=prev)
        else:
            var[name] = s64.combine(p, m, v, it, T[torch.float64], field.K, torch.float64, variant=name, g_prev=g_prev, reg_params=render_params)
    _cache[(mode, k)] = dict(z=z, it=it, ref=ref, r32=r32, r32b=r32b, var=var, before=(p, m, v), after=_state(z, k, "after"), field=field, cfg2=cfg2,
                             kept_own=kept_own, render_params=render_params, nb=nb)
    return _cache[(mode, k)]


def _b1b2():
    return float(np.float32(s64.B1)), float(np.float32(s64.B2))


def _recover(m_after, m_before):
    b1, _ = _b1b2()
    return (np.asarray(m_after, np.float64) - b1 * np.asarray(m_before, np.float64)) / (1.0 - b1)


def _eps_rows(c, n):
    """bool mask over tensor n: the rows of a time plane that are the base keyframe row of no render of the iteration (see the docstring)"""
    shape = c["before"][0][n].shape
    out = np.zeros(shape, bool)
    if "plane_time" in n:
        K = shape[2]
        real = {int(round((r["plan"]["tn_base"] + 1) / 2 * (K - 1))) for r in c["ref"]["renders"]}
        for r in range(K):
            if r not in real:
                out[:, :, r, :] = True
    return out


def _derive(c):
    """B[family], B_p, the exempt sets and the value bounds of one case, from the yardstick's float32 and float64 evaluations alone"""
    ref, r32 = c["ref"], c["r32"]
    evals = [r for r in (r32, c.get("r32b")) if r is not None]
    p, m, v = c["before"]
    B = dict.fromkeys(s64.FAMILIES, 0.0)
    fig, out32 = {}, {}
    for n in p:
        g = ref["grads"][n]
        if n in s64.FAMILY and np.abs(g).max() > 0:
            e = max(_metric(_recover(r["m"][n], m[n]), g) for r in evals)
            fig[n] = e
            B[s64.FAMILY[n]] = max(B[s64.FAMILY[n]], 3.0 * e)
    # The appearance branch (render MLP, basis_mat, appearance planes) adds one contribution per masked sample with fp32 atomics, per 32-sample
    # tile; torch's float32 sums are blocked and stay five to ten times under a sequential sum of that length.  A sequential fp32 sum of N terms of
    # one sign carries a relative error of u sqrt(N / 3) (a random walk of roundings u = 2^-24 on partial sums that grow linearly); renderModule.
    # mlp.4.bias, three elements that are exactly such a sum and that no ReLU kink touches (render64's kink bracket moves it by 1e-9), shows it:
    # device 3.0e-6 - 3.7e-6, float32 yardstick 9.5e-7, u sqrt(N / 3) = 9.2e-6 at N = 72 000.  Three times that term is the floor of B in the two
    # families - from the format and the yardstick's own sample count, not from the device
    n_app = float(sum(int(r["app_mask"].sum()) for r in ref["renders"]))
    b_red = 3.0 * 2.0 ** -24 * np.sqrt(n_app / 3.0)
    B32 = dict(B)
    for f in ("mlp", "app"):
        B[f] = max(B[f], b_red)
    for n in fig:       # what the float32 evaluations themselves leave outside assert_grad's element-wise check at this bound
        bn = max(B[s64.FAMILY[n]], APP_TIME_B) if n.startswith("app_plane_time.") else B[s64.FAMILY[n]]
        out32[n] = max(outfrac(_recover(r["m"][n], m[n]), ref["grads"][n], 20 * bn) for r in evals)
    # the upper limit per family, a third of the smallest move that a wrong variant (d), (e), (f), (g) makes in it, is measured and printed; B is
    # the LOWER limit.  One class has a bound of its own: APP_TIME_B (above) for the appearance time planes
    Blow, upper = dict(B), {}
    for name in ("d", "e", "f1", "f2", "g"):
        if name in c["var"]:
            mv = {}
            for n in fig:
                e = _metric(c["var"][name]["grads"][n], ref["grads"][n])
                if e > 0:
                    mv[s64.FAMILY[n]] = max(mv.get(s64.FAMILY[n], 0.0), e)
            for f, e in mv.items():
                upper[f] = min(upper.get(f, np.inf), e / 3.0)
    Bn = {n: (max(B[s64.FAMILY[n]], APP_TIME_B) if n.startswith("app_plane_time.") else B[s64.FAMILY[n]]) for n in fig}
    exempt, share = {}, {}
    for n in p:
        g = ref["grads"][n]
        fam = s64.FAMILY.get(n)
        ex = np.zeros(g.shape, bool)
        if fam is not None and np.abs(g).max() > 0:
            ex = (np.abs(g) < B32[fam] * np.abs(g).max()) & (g != 0)      # (by 3 x the float32 figure alone: the smaller set)
        exempt[n] = ex
        share[n] = float(ex.mean())
        share_eps = float((ex & _eps_rows(c, n)).mean())
        if share_eps:
            fig[("eps rows", n)] = share_eps
    lr = {n: ref["schedule"]["lr_plane" if "plane" in n else "lr_net"] for n in p}
    Bp, worst = 0.0, ""
    for n in p:
        for r in evals:
            e = np.abs((np.asarray(r["p"][n], np.float64) - p[n]) - (ref["p"][n] - p[n]))[~exempt[n]] / lr[n]
            if e.size and 3.0 * float(e.max()) > Bp:
                Bp, worst = 3.0 * float(e.max()), n
    vb = dict(loss=optim64.bound(r32["mse"][-1], ref["mse"][-1]), L1=optim64.bound(r32["regs"][0], ref["regs"][0]),
              TVd=optim64.bound(r32["regs"][1], ref["regs"][1]), TVa=optim64.bound(r32["regs"][2], ref["regs"][2]))
    if not c["cfg2"] and ref["n_kept"]:
        vb["lv"] = optim64.bound(r32["lv"], ref["lv"])
    return dict(B=B, Bp=Bp, Bp_tensor=worst, exempt=exempt, share=share, lr=lr, value=vb, fig=fig, out32=out32, Blow=Blow, upper=upper, Bn=Bn, B32=B32, b_red=b_red)


def _record(c, sched):
    """the fp32 scalars a record-mode iteration uploads for a schedule: the loss weights (rec[2:6]; three on the radiance-only workload) and Adam's
    1 / sqrt(1 - b2^t), lr_k / (1 - b1^t) per stepped tensor (rec[16:]), formed as Adam.next_hyper forms them"""
    b1, b2 = _b1b2()
    t = sched["t_bias"]
    bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
    names = [str(n) for n in c["z"]["names"]]
    w = sched["w"][:3 if c["cfg2"] else 4]
    hyper = [1.0 / np.sqrt(bc2)] + [float(np.float32(sched["lr_plane" if "plane" in n else "lr_net"])) / bc1 for n in names]
    return np.array(list(w) + hyper, np.float32)


def _variant_moves(c, D):
    """per wrong variant: the largest move of a gradient tensor over its family's bound, and of the update over B_p"""
    ref = c["ref"]
    p = c["before"][0]
    out = {}
    for name, vr in c["var"].items():
        gmove = 0.0
        for n in p:
            g = ref["grads"][n]
            if n in D["Bn"] and D["Bn"][n] > 0:
                gmove = max(gmove, _metric(vr["grads"][n], g) / D["Bn"][n])
        pmove = 0.0
        for n in p:
            e = np.abs(vr["p"][n] - ref["p"][n])[~D["exempt"][n]] / D["lr"][n]
            if e.size and D["Bp"] > 0:
                pmove = max(pmove, float(e.max()) / D["Bp"])
        # the record modes: would the scalars this variant uploads (fp32: rec[2:6] and rec[16:]) differ from the right ones?
        rec = str(c["z"]["mode"]) in RECORD_MODES and not np.array_equal(_record(c, vr["schedule"]), _record(c, ref["schedule"]))
        # the update from the device's own moments is formed with the yardstick's lr_t and bias corrections: a driver that followed the variant would
        # leave it by the ratio of the two step sizes (tolerance: five fp32 roundings, 5e-7; counted from 1e-6 on)
        b1, b2 = _b1b2()
        sv, sr = vr["schedule"], ref["schedule"]
        ratio = max(abs(sv[q] / (1.0 - b1 ** float(sv["t_bias"])) / (sr[q] / (1.0 - b1 ** float(sr["t_bias"]))) - 1.0) for q in ("lr_plane", "lr_net"))
        ratio = max(ratio, abs(np.sqrt((1.0 - b2 ** float(sr["t_bias"])) / (1.0 - b2 ** float(sv["t_bias"]))) - 1.0))
        out[name] = dict(grad=gmove, update=pmove, record=rec, own=ratio > 1e-6)
    return out


def _check(mode, k):
    """everything is measured and printed first, then asserted"""
    c = _case(mode, k)
    z, ref, r32 = c["z"], c["ref"], c["r32"]
    D = _derive(c)
    p0, m0, v0 = c["before"]
    p1, m1, v1 = c["after"]
    b1, b2 = _b1b2()
    label = f"{mode}:it{c['it']}"
    bad = []

    def check(ok, *what):
        if not ok:
            bad.append((label,) + what)

    # ---- maps
    maps = []
    for b in range(c["nb"]):
        r = ref["renders"][b]
        err = np.abs(z[f"it{k}:rgb{b}"].astype(np.float64) - r["rgb"])
        e32 = np.abs(r32["rgb"][b].astype(np.float64) - r["rgb"])
        maps.append((float(err.max()), float((err - FP32_FLOOR["rgb"] - MAP_RTOL * np.abs(r["rgb"])).max()),
                     float((e32 - FP32_FLOOR["rgb"] - MAP_RTOL / 3 * np.abs(r["rgb"])).max())))
    # ---- values
    vals = dict(loss=(float(z[f"it{k}:loss"]), ref["mse"][-1]), L1=(float(z[f"it{k}:regs"][0]), ref["regs"][0]),
                TVd=(float(z[f"it{k}:regs"][1]), ref["regs"][1]), TVa=(float(z[f"it{k}:regs"][2]), ref["regs"][2]))
    if "lv" in D["value"]:
        vals["lv"] = (float(z[f"it{k}:lv"]), ref["lv"])
    verr = {q: abs(a - b) / abs(b) for q, (a, b) in vals.items()}
    # ---- gradients, second moments, update
    gerr, verr2, perr = {}, {}, {}
    fam_dev = dict.fromkeys(s64.FAMILIES, 0.0)
    for n in p0:
        g = ref["grads"][n]
        gd = _recover(m1[n], m0[n])
        if n in s64.FAMILY and np.abs(g).max() > 0:
            gerr[n] = _metric(gd, g)
            fam_dev[s64.FAMILY[n]] = max(fam_dev[s64.FAMILY[n]], gerr[n])
            vref = b2 * v0[n].astype(np.float64) + (1 - b2) * g * g
            verr2[n] = (_metric(v1[n], vref), optim64.ulp_floor(vref))
        d = np.abs((p1[n].astype(np.float64) - p0[n]) - (ref["p"][n] - p0[n])) / D["lr"][n]
        ex = D["exempt"][n]
        perr[n] = (float(d[~ex].max()) if (~ex).any() else 0.0, float(np.abs(p1[n].astype(np.float64) - p0[n])[ex].max() / D["lr"][n]) if ex.any() else 0.0)
    moves = _variant_moves(c, D)
    worst_p = max((e[0], n) for n, e in perr.items())
    print(f"[step64] {label}: maps (max abs err, excess, float32 excess at a third) {maps}; values rel err "
          + ", ".join(f"{q} {e:.1e} (bound {D['value'][q]:.1e})" for q, e in verr.items())
          + f"; gradient 3 x float32 / B (reduction floor {D['b_red']:.1e}) / a third of the nearest variant / device: "
          + ", ".join(f"{f} {D['B32'][f]:.1e} / {D['B'][f]:.1e} / {D['upper'].get(f, float('nan')):.1e} / {fam_dev[f]:.1e}" for f in s64.FAMILIES)
          + f"; app_plane_time device {max([gerr[n] for n in gerr if n.startswith('app_plane_time.')] or [0.0]):.1e}"
          + f"; update B_p {D['Bp']:.1e} ({D['Bp_tensor']}) / device {worst_p[0]:.1e} ({worst_p[1]})"
          + "; exempt share, largest: " + "{:.2%} ({})".format(*max((s, n) for n, s in D["share"].items()))
          + "; variants (gradient / B, update / B_p): " + ", ".join(f"{q} {mv['grad']:.1f} / {mv['update']:.1f}" for q, mv in moves.items()), flush=True)
    for b, (emax, excess, e32) in enumerate(maps):
        check(e32 <= 0, "render", b, "the float32 evaluation does not keep a third of MAP_RTOL")
        check(excess <= 0, "render", b, "rgb max abs err", emax)
    for q, e in verr.items():
        check(e <= D["value"][q], "value", q, e, D["value"][q])
    # ---- counters and masks
    for b in range(c["nb"]):
        r, cnt = ref["renders"][b], z[f"it{k}:counters{b}"]
        nsteps = len(r["plan"]["steps"])
        masked = int(r["app_mask"].sum())
        check(int(cnt[0]) == int(r["valid"].sum()), "render", b, "valid count", int(cnt[0]), int(r["valid"].sum()))
        check(int(cnt[1]) == (int(r["in_gate"].sum()) if nsteps else 0), "render", b, "RK2 list", int(cnt[1]), int(r["in_gate"].sum()))
        check(int(cnt[7]) == 0, "render", b, "a device-side time left its captured plan")
        if f"it{k}:mask{b}" in z:
            check(int(cnt[2]) == masked, "render", b, "masked count", int(cnt[2]), masked)
            check(len(r["flips"]) <= 1e-3 * masked, "render", b, "mask flips", len(r["flips"]), masked)
            check((r["flip_dist"] <= 2e-6).all(), "render", b, "a differing sample is not at the threshold")
        else:
            check(False, "render", b, "the device's mask is not observable: forward() of the same rays masked another count than", int(cnt[2]))
        if not c["cfg2"] and b == 0:
            check(nsteps >= 1, "render 0 is the non-keyframe render")
    if not c["cfg2"]:
        kept, dist = c["kept_own"]
        n_dev = int(round(float(z[f"it{k}:pde_out"][1])))
        check(f"it{k}:kept" in z, "the device's kept set is not observable")
        if f"it{k}:kept" in z:
            diff = z[f"it{k}:kept"] != kept
            print(f"[step64] {label}: PDE kept {n_dev} of {kept.size}; differs from kept64 on {int(diff.sum())} points"
                  + (f", farthest {dist[diff].max():.1e} from the threshold" if diff.any() else ""))
            check(int(z[f"it{k}:kept"].sum()) == n_dev == ref["n_kept"], "kept count", n_dev, ref["n_kept"])
            check(diff.sum() <= max(1, 1e-3 * n_dev), "kept set differs from kept64 on", int(diff.sum()))
            check(not diff.any() or dist[diff].max() <= 2e-6, "a differing point is not at the threshold")
        check(n_dev > 64, "the PDE term keeps too few points to mean anything", n_dev)
    # ---- gradients and moments
    for n in p0:
        g = ref["grads"][n]
        if n in gerr:
            try:
                # (element-wise: never less than the default share, nor than 3 x what the float32 evaluations themselves leave outside - the
                #  recovery from fp32 moments costs an element with a large history and a small gradient its digits)
                assert_grad(_recover(m1[n], m0[n]), g, D["Bn"][n], f"{label}:{n}",
                            out_max=max(5e-3, 4.0 / g.size, 3.0 * D["out32"][n]))
            except AssertionError as e:
                bad.append((label, "gradient", n, str(e), "float32 figure", D["fig"][n]))
            e, fl = verr2[n]
            check(e <= 2 * D["Bn"][n] + fl, "exp_avg_sq", n, e, 2 * D["Bn"][n] + fl)
        quiet = (g == 0) & (m0[n] == 0) & (v0[n] == 0)
        if quiet.any():
            check(np.array_equal(p1[n][quiet], p0[n][quiet]) and not m1[n][quiet].any() and not v1[n][quiet].any(), "zero gradient, no history, yet moved", n)
        check(perr[n][0] <= D["Bp"], "update", n, perr[n][0], D["Bp"])
        check(perr[n][1] <= 1.001 / (1 - b1), "update of an exempt element", n, perr[n][1])
        # the last line of Adam from the device's OWN moments, every element (the exempt ones too): p1 = p0 - s m1 / (sqrt(v1) c + eps) evaluated in
        # float64 from fp32 inputs; an fp32 evaluation of its five operations is within 5 x 2^-24 of it, and storing p costs half a spacing of p
        t = ref["schedule"]["step"]
        lr32 = float(np.float32(D["lr"][n]))
        dp_own = -(lr32 / (1.0 - b1 ** float(t))) * m1[n].astype(np.float64) / (np.sqrt(v1[n].astype(np.float64)) / np.sqrt(1.0 - b2 ** float(t)) + float(np.float32(s64.EPS)))
        tol = 8.0 * 2.0 ** -24 * np.abs(dp_own) + 0.5 * np.spacing(np.maximum(np.abs(p0[n]), np.abs(p1[n])).astype(np.float32)).astype(np.float64)
        over = np.abs((p1[n].astype(np.float64) - p0[n]) - dp_own) - 1.001 * tol
        check(float(over.max()) <= 0, "update from the device's own moments", n, float(over.max()), float(np.abs(dp_own).max()))
    # ---- buffers, schedule
    check(int(z[f"it{k}:flat_nonzero_bits"]) == 0, "the flat gradient buffer is not all zero bits after the step")
    s = ref["schedule"]["after"]
    nsched = 3 if c["cfg2"] else 4
    check(np.allclose(z[f"it{k}:sched"][:nsched], s["w"][:nsched], rtol=1e-14, atol=0), "loss weights after the iteration", z[f"it{k}:sched"], s["w"])
    names = [str(n) for n in z["names"]]
    check(np.all(z[f"it{k}:adam_step"] == s["step"]), "Adam's step count", z[f"it{k}:adam_step"][:3], s["step"])
    lrs = np.unique(z[f"it{k}:lr"])
    check(np.allclose(np.sort(lrs), sorted({s["lr_net"], s["lr_plane"]}), rtol=1e-14, atol=0), "learning rates after the iteration", lrs)
    if f"it{k}:rec_head" in z:
        rec = z[f"it{k}:rec_head"]
        nw = 3 if c["cfg2"] else 4
        want = _record(c, ref["schedule"])
        check(np.array_equal(rec[2:2 + nw], want[:nw]), "rec[2:6], the loss weights the device read", rec[2:6], want[:nw])
        check(np.array_equal(rec[16:16 + len(want) - nw], want[nw:]), "rec[16:], the Adam scalars the device read")
        check(np.array_equal(z[f"it{k}:t_rec"].astype(np.float32), z[f"it{k}:t"].astype(np.float32)), "rec[0:2] against the host's times", z[f"it{k}:t_rec"], z[f"it{k}:t"])
    if mode == "cfg2_eager":
        check(z[f"it{k}:reg_on_side_stream"].size == 1 and bool(z[f"it{k}:reg_on_side_stream"].all()), "the regulariser pass did not take the early side stream")
    if mode == "shadow3":
        for n in names:
            check(np.array_equal(z[f"it{k}:after:field:{n}"], z["it0:before:field:" + n]), "shadow3 moved the field's own", n)
    for b in bad:
        print("[step64] FAILED", str(b)[:600], flush=True)
    assert not bad, bad
    return D, moves


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_iteration_matches_float64(mode, k):
    _check(mode, k)
    print(f"[step64] wall time of the file up to {mode}:{k}: {time.time() - _T0:.0f} s")


def test_modes_see_the_same_draws():
    zs = {m: _worker(m) for m in SAME_DRAWS}
    base = zs[SAME_DRAWS[0]]
    for m, z in zs.items():
        for k in range(3):
            for key in ("o0", "d0", "tg0", "u0", "o1", "d1", "tg1", "u1", "pts", "pt"):
                a, b = z[f"it{k}:{key}"], base[f"it{k}:{key}"]
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (m, k, key, "drew something else than", SAME_DRAWS[0])
            assert np.array_equal(z[f"it{k}:t"].astype(np.float32).view(np.uint32), base[f"it{k}:t"].astype(np.float32).view(np.uint32)), (m, k, "times")


def test_exempt_share_stays_under_the_cap():
    """from the yardstick alone: at most 2 % of any tensor of 64 or more elements is exempt - or, for the tensors of OVER_CAP, at most its ceiling"""
    worst = {}
    for mode in MODES:
        for k in range(3):
            c = _case(mode, k)
            D = _derive(c)
            for n, sh in D["share"].items():
                if c["before"][0][n].size >= 64 and sh > worst.get(n, (0.0,))[0]:
                    worst[n] = (sh, f"{mode}:it{c['it']}", D["fig"].get(("eps rows", n), 0.0), c["before"][0][n].size)
    print("[step64] largest exempt share per tensor (share, where, of which rows of a time plane beside a base row, elements):", flush=True)
    for n, w in worst.items():
        print(f"[step64] share {n} {w[0]:.4f} {w[1]} {w[2]:.4f} {w[3]}", flush=True)
    over = {n: w[:2] for n, w in worst.items() if w[0] > OVER_CAP.get(n, EXEMPT_CAP)}
    assert not over, over
    stale = [n for n in OVER_CAP if worst.get(n, (0.0,))[0] <= EXEMPT_CAP]
    assert not stale, ("listed in OVER_CAP but under the cap everywhere", stale)


def _kind(mode):
    return "record" if mode in RECORD_MODES else "eager"


def test_every_wrong_variant_is_seen():
    """from the yardstick alone: each wrong variant moves some asserted observable of some iteration by 3 x its bound or more - per kind of mode
    (the record modes also assert the scalars the device read) - or is listed in BLIND for that kind, and then it is blind"""
    seen = {}
    for mode in MODES:
        for k in range(3):
            c = _case(mode, k)
            for name, mv in _variant_moves(c, _derive(c)).items():
                key = (_kind(mode), name)
                how = [w for w, ok in (("gradient", mv["grad"] >= 3.0), ("update", mv["update"] >= 3.0), ("record", mv["record"]), ("own moments", mv["own"])) if ok]
                seen.setdefault(key, set()).update(how)
    print("[step64] what sees each wrong variant:", {f"{a}:{b}": sorted(v) for (a, b), v in sorted(seen.items())})
    for key, how in seen.items():
        if key in BLIND:
            assert not how, (key, "is listed as blind but is seen by", how)
        else:
            assert how, (key, "no asserted observable sees this variant")
    assert {b for _, b in seen} == set(s64.VARIANTS)
