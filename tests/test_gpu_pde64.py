"""The PDE term on the device (get_vel_loss: the occupancy prefilter, the Jacobian forward, k_pde_fuse_bwd and the weight-gradient reduction)
against its float64 restatement (tests/pde64.py, pinned to the reference's goldens by tests/test_pde64_golden.py) on the device's own kept set.

Cases (tests/pde64_worker.py): the headline shape (the bench field, P = 262 144, a moving velocity field); field B, which keeps every point, at
kept counts that sit on the kernel's edges - partial tiles and 128-point workgroups (1, 31, 33, 127, 129), the workgroup grants of k_pde_fuse_bwd,
and one 262 144-point chunk exactly, a second chunk holding one point, two and three chunks; and large pre-activations.
The grant depends on the call (pde.hip, pde_fused_adjoint): a split call - get_vel_loss with the default NVFI_PDE_SPLIT=1 and P <= 262 144 -
grants PDE_NSLAB - 8 = 248 workgroups; NVFI_PDE_SPLIT=0, the multi-chunk calls and nvfi_pde_loss_ex without a second stream grant 256.  So
under the defaults 32 x 248 and 32 x 248 + 1 points fill the 248 grant exactly and go one tile over it (32 x 256 + 5 is nine tiles over it), and
the one_stream setting runs 32 x 256 and 32 x 256 + 5 points: the 256 grant filled exactly and one partial tile over it.  The worker records
whether each call met that condition (the field's pde_split and P), and the test asserts it per setting.  Every NVFI_* switch that changes
the PDE path runs in a process of its own on the headline, 248 / 249-tile and two-chunk cases.

Large pre-activations: both nets' first layer x 2.5 and hidden layers x 4 (the issue's x 2.5 on the hidden layers reaches |z| of 5 only), so |z|
reaches 25-35: the tails of SiLU'' and dead ReLU units.  The parameter gradient of the ReLU net jumps where a unit crosses its kink, and fp32 and
float64 may take different sides within rounding of it (at ~0.2 % of the points that moved a gradient by up to 3.7e-4 of its peak), so the points
within 4 x the worst-case fp32 rounding bound of a kink (~6 %) are redrawn: this case does NOT check the kernels' behaviour AT a kink, only
around it.

Bounds: loss rel err <= 1e-5; Jacobian rows 0-2 rtol 1e-5, atol 1e-6 x max|J|; every gradient tensor max(maxrel, rel_l2) <= B.  Each large case
checks that the bound can see a dropped tile: removing the last full 32-point tile of the kept set moves some tensor of the float64 reference by
>= 3 B.  Each small case checks that removing the last kept point moves it by more than B.

Measured on one MI355X (defaults; the switches agree to within 2x): worst gradient error 1.4e-7 - 2.8e-7 up to 34 k kept points (headline
34 171 kept: 1.8e-7, one-tile shift 1.0e-3), 4.6e-6 at 262 144, 7.3e-6 at 262 145, 1.1e-6 at 266 277 and 1.8e-6 at 528 421 kept points (the
acceleration net's hidden layers: fp32 slab sums and the occasional ReLU unit within rounding of its kink); on the 256 grant (one_stream)
1.6e-7 at 32 x 256 and 32 x 256 + 5 points; loss <= 3e-7, Jacobian <= 3.3e-6.
The one-tile shift at 528 421 kept points is 5.1e-5, so B = 1.5e-5 (the issue's starting value 2e-5 could not see a dropped tile there).
The file takes about 35 s (seven worker processes).  A mutation of pde_pass_count (pde.h; then pf_count of pde_fuse.hip) that drops the last
kept point of a pass whenever more than 32 are left fails the 129-point, 249-tile and partial-gradient cases here; every older PDE test passed
on it.  The unfused_launch setting also pins the call's bookkeeping (out[1..3], the counters: pde.h's writers) to the defaults' values."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pde64
from conftest import ROOT, assert_grad, maxrel, rel_l2

pytestmark = pytest.mark.gpu

B = 1.5e-5
SMALL = ["B1", "B31", "B33", "B127", "B129"]
LARGE = ["head", "B7936", "B7937", "B8197", "B262144", "B262145", "B528421", "bigz"]
SWITCH_CASES = ["head", "B7936", "B7937", "B266277"]
EXTRA_CASES = {"one_stream": ["B8192", "B8197"]}      # the 256-workgroup grant, filled exactly and one partial tile over it
SWITCHES = {"deterministic": dict(NVFI_DETERMINISTIC="1"), "pde_unfused": dict(NVFI_PDE_FUSE="0"), "jet_fp32": dict(NVFI_PDE_JET_X6="0"),
            "unfused_launch": dict(NVFI_FUSED_LAUNCH="0"), "one_stream": dict(NVFI_PDE_SPLIT="0"), "prefilter_fp32": dict(NVFI_PDE_PREFILTER="fp32")}

_runs = {}
_failed = []
_refs = {}


def _worker(tag, cases, env):
    """one worker process per switch setting; after a failed one no further worker is started"""
    if tag in _runs:
        return _runs[tag]
    if _failed:
        pytest.fail(f"not run: the worker of {_failed[0]} failed")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"pde64_{os.getpid()}_{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pde64_worker.py"), out, ",".join(cases)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        _failed.append(tag)
        pytest.fail(f"worker {tag} exited with {r.returncode}:\n" + r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    _runs[tag] = {k: z[k] for k in z.files}
    os.remove(out)
    return _runs[tag]


def _defaults():
    return _worker("defaults", SMALL + LARGE + ["B266277", "abi7937"], {})


def _params(z, kind):
    import torch
    return pde64.as_params([z[f"model:{kind}:p{i}"] for i in range(24)], "cuda" if torch.cuda.is_available() else "cpu")


def _reference(z, case, n_jac=64):
    """float64 pde64 of the device's kept set, cached by model, inputs and kept mask"""
    kind = str(z[f"{case}:model"])
    h = hashlib.sha1()
    for k in (f"{case}:points", f"{case}:t", f"{case}:kept"):
        h.update(np.ascontiguousarray(z[k]).tobytes())
    for i in range(24):
        h.update(np.ascontiguousarray(z[f"model:{kind}:p{i}"]).tobytes())
    key = h.hexdigest()
    if key not in _refs:
        ps = _params(z, kind)
        _refs[key] = (pde64.pde64(z[f"{case}:points"], z[f"{case}:t"], z[f"{case}:kept"], ps, z[f"model:{kind}:aabb"], n_jac=n_jac), ps)
    return _refs[key]


def _metric(a, b):
    return max(maxrel(a, b), rel_l2(a, b))


def _check(z, case, label, want=None):
    """everything is measured and printed first, then asserted"""
    ref, ps = _reference(z, case)
    n = int(z[f"{case}:n_kept"])
    P = z[f"{case}:points"].shape[0]
    lerr = abs(float(z[f"{case}:loss"]) - ref["loss"]) / abs(ref["loss"])
    m = min(64, n)
    J = z[f"{case}:jac"][:m, :3].astype(np.float64) if f"{case}:jac" in z else None
    Jr = ref["jac"][:m]
    asked = [i for i in range(24) if want is None or i in want]
    errs = {pde64.NAMES[i]: _metric(z[f"{case}:g{i}"], ref["grads"][pde64.NAMES[i]]) for i in asked}
    worst = max((e, k) for k, e in errs.items())
    # the self-check: the bound must see one tile less (large cases) / the last point less (small cases)
    if n >= 256:
        t0 = (n // 32 - 1) * 32
        s, sl = pde64.shift(ref, ps, np.arange(t0, t0 + 32), _metric)
        what, need = "one-tile shift", 3 * B
    else:
        # (one kept point: dropping it leaves nothing and the device's gradients would all be zero, which the gradient check sees)
        s, sl = pde64.shift(ref, ps, np.array([n - 1]), _metric) if n > 1 else (np.inf, np.inf)
        what, need = "last-point shift", B
    jerr = float(np.max(np.abs(J - Jr) / (np.abs(Jr) + 0.1 * np.abs(Jr).max()))) if J is not None else 0.0
    print(f"[pde64] {label}: kept {n} of {P}, loss rel err {lerr:.2e}, Jacobian err {jerr:.2e}, worst gradient err {worst[0]:.2e} ({worst[1]}), "
          f"{what} {s:.2e} (loss {sl:.2e}), bound B = {B:g}")
    assert n == ref["n_kept"], (label, n, ref["n_kept"])
    if f"{case}:split" in z:        # which workgroup grant the adjoint met (see the module docstring)
        split_expected = not label.startswith("one_stream:") and P <= 262144
        assert bool(z[f"{case}:split"]) == split_expected, (label, "split call", bool(z[f"{case}:split"]))
    if str(z[f"{case}:model"]) in ("B", "bigz"):
        assert n == P, (label, "field B keeps every point", n, P)
    assert lerr <= 1e-5, (label, "loss", lerr)
    if J is not None:
        np.testing.assert_allclose(J, Jr, rtol=1e-5, atol=1e-6 * np.abs(Jr).max(), err_msg=label)
    for i, name in enumerate(pde64.NAMES):
        if i in asked:
            assert_grad(z[f"{case}:g{i}"], ref["grads"][name], B, f"{label}:{name}")
        else:
            assert float(np.abs(z[f"{case}:g{i}"]).max()) == 0.0, (label, name, "asked not to be written")
    assert (s >= need) if n >= 256 else (s > need), (label, what, s, need)
    return worst[0]


@pytest.mark.parametrize("case", SMALL + LARGE + ["B266277"])
def test_pde_matches_float64(case):
    z = _defaults()
    _check(z, case, f"defaults:{case}")


def test_large_preactivations_reach_the_activation_tails():
    """the bigz case has |z| of 20-40 in the hidden layers (SiLU'' ~ 1e-8 there, and ReLU units that are dead for most points)"""
    import torch
    z = _defaults()
    ps = _params(z, "bigz")
    ref, _ = _reference(z, "bigz")
    q = torch.cat([ref["xn"], ref["t"][:, None]], 1)[ref["idx"][:4096]].to(ps[0].device, torch.float64)
    for off, act in ((0, torch.nn.functional.silu), (12, torch.relu)):
        enc = [q] + [f(q * 2.0 ** k) for k in range(3) for f in (torch.sin, torch.cos)]
        h = torch.cat(enc, 1)
        zmax = 0.0
        for i in range(5):
            zz = torch.nn.functional.linear(h, ps[off + 2 * i], ps[off + 2 * i + 1])
            zmax = max(zmax, float(zz.abs().max()))
            h = act(zz)
        assert 20.0 <= zmax <= 80.0, (off, zmax)


def test_two_chunk_cases_do_reach_the_later_chunks():
    z = _defaults()
    assert int(z["B262145:n_kept"]) == 262145 and int(z["B528421:n_kept"]) > 2 * 262144 and int(z["B266277:n_kept"]) > 262144


def _bookkeeping_matches_the_fused_launch(z, zd):
    """out[] and the counters are written by pde.h's writers from two callers: the last workgroup of k_pde_seeds (defaults) and the stand-alone
    k_pde_pass_count / k_pde_finish / k_pde_counters launches (NVFI_FUSED_LAUNCH=0).  On the cases both workers run, the integers (the eight
    counters, the kept count in out[1]) are equal exactly; out[2], out[3] (sum div^2, sum transport^2) are accumulated with atomics in an
    order that differs from run to run and agree within the loss bound.  B266277 is the two-chunk case: the ticket is drawn from zero again
    in the second pass, or out[] is never written."""
    for case in SWITCH_CASES:
        cu, cf = z[f"{case}:counters"], zd[f"{case}:counters"]
        ou, of = z[f"{case}:out"].astype(np.float64), zd[f"{case}:out"].astype(np.float64)
        rel = np.abs(ou[2:4] - of[2:4]) / np.abs(of[2:4])
        print(f"[pde64] unfused_launch vs defaults, {case}: counters {cu.tolist()} / {cf.tolist()}, out[1] {ou[1]:.0f} / {of[1]:.0f}, "
              f"sums rel diff {rel[0]:.2e}, {rel[1]:.2e}")
        assert cu.shape == (8,) and cu.dtype == np.int64 and np.array_equal(cu, cf), (case, cu, cf)
        assert int(cu[1]) == z[f"{case}:points"].shape[0] and int(cu[4]) == int(z[f"{case}:n_kept"]), (case, cu)
        assert ou[1] == of[1] == float(z[f"{case}:n_kept"]), (case, ou[1], of[1])
        assert (rel <= 1e-5).all(), (case, "sum div^2 / sum transport^2", rel)


@pytest.mark.parametrize("setting", list(SWITCHES))
def test_pde_switch_matches_float64(setting):
    cases = SWITCH_CASES + EXTRA_CASES.get(setting, [])
    z = _worker(setting, cases, SWITCHES[setting])
    bad = []
    for case in cases:
        try:
            _check(z, case, f"{setting}:{case}")
        except AssertionError as e:
            bad.append(f"{case}: {e}")
    assert not bad, bad
    if setting == "unfused_launch":
        _bookkeeping_matches_the_fused_launch(z, _defaults())


@pytest.mark.parametrize("drop", ["accel", "layer2"])
def test_pde_c_abi_partial_gradient_sets_match_float64(drop):
    """nvfi_pde_loss_ex with the acceleration net's slots (fused kernel's first half only) or weight_net's second hidden layer (the unfused
    adjoint) left NULL, on the 249-tile case: the tensors that are asked for meet B against float64, the others stay zero"""
    z = _defaults()
    skip = set(range(12, 24)) if drop == "accel" else {4, 5}
    _check(z, f"abi7937_{drop}", f"abi:{drop}", want=set(range(24)) - skip)
