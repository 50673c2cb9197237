"""Characteristic loss, CPU side: the float64 yardstick (tests/char64.py) against goldens made from the reference's pieces
(tests/golden/make_golden_charloss.py), and the presence of the feature at every layer (ABI, binding, field methods)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import char64 as c64
from conftest import GOLD
from helpers import load_meta

CASES = {"A": ("k1", "kmax", "up", "zero", "neg", "snap0"), "B": ("k1", "kmax", "up", "zero", "neg", "snap0", "out")}


@pytest.fixture(scope="module")
def gc():
    return np.load(os.path.join(GOLD, "charloss.npz"))


def golden_params(kind):
    """the 13 tensors of a golden field (B shares basis_mat with A)"""
    meta, sd = load_meta(kind)
    if kind == "B":
        for k, v in load_meta("A")[1].items():
            sd.setdefault(k, v)
    return c64.params_from_sd(sd), int(meta["num_keyframes"]), float(meta["tmax"])


@pytest.mark.parametrize("kind", ["A", "B"])
def test_char64_reproduces_reference_goldens(gc, kind):
    """tolerance per quantity: the reference's own fp32 error against the yardstick, stored beside the goldens, times 2 (the goldens are
    fp32 values, the yardstick is not)"""
    params, K, tmax = golden_params(kind)
    for case in CASES[kind]:
        key = f"{kind}:{case}"
        t_k, row = c64.snap_time(K, tmax, float(gc[key + ":t"]))
        assert t_k == float(gc[key + ":t_k"]) and row == int(gc[key + ":row"]), key
        full = case == "kmax"
        y = c64.char64(params, K, gc[key + ":points"], gc[key + ":points0"], row)
        for q in c64.TERMS:
            e, tol = c64.rel_err(y[q], gc[f"{key}:{q}"]), 2 * float(gc[f"{key}:ref32_err:{q}"])
            print(f"{key} {q}: rel err {e:.2e} (bound {tol:.2e})")
            assert e <= tol, (key, q, e, tol)
        for n in c64.NAMES:
            tol = 2 * float(gc[f"{key}:ref32_err:grad:{n}"])
            if full:
                e = c64.rel_err(y["grads"][n], gc[f"{key}:grad:{n}"])
                assert e <= tol, (key, n, e, tol)
            # the L2 norm of a tensor moves by at most sqrt(size) x the max-norm error of its entries
            norm, ref = float(np.linalg.norm(y["grads"][n])), float(gc[f"{key}:gradnorm:{n}"])
            assert abs(norm - ref) <= tol * np.sqrt(y["grads"][n].size) * np.abs(y["grads"][n]).max() + 1e-30, (key, n, norm, ref)
        if row == 0:
            assert y["loss_d"] == 0.0 and y["loss_a"] == 0.0 and all(not g.any() for g in y["grads"].values())


def test_golden_point_sets_meet_their_conditions(gc):
    for kind, case in (("A", "kmax"), ("B", "out")):
        frac = c64.outside_fraction(gc[f"{kind}:{case}:points0"])
        assert 0.01 <= frac <= 0.5, (kind, case, frac)
    for kind in ("A", "B"):
        assert (np.abs(gc[f"{kind}:kmax:points"]) == 1).any()


def test_exports_listed_and_built():
    from nvfi_amd import _lib
    for name in ("nvfi_char_loss", "nvfi_char_workspace_bytes"):
        assert name in _lib.EXPORTS, name
    assert os.path.exists(_lib.SO), "libnvfi_hip.so has not been built"
    L = ctypes.CDLL(_lib.SO)
    for name in ("nvfi_char_loss", "nvfi_char_workspace_bytes"):
        assert hasattr(L, name), name
    assert L.nvfi_abi_version() == 5


def test_field_methods_exist_and_refuse_the_cpu():
    from helpers import make_model
    from nvfi_amd import _lib
    from nvfi_amd.models.tensorf_keyframe import TensorVMKeyframeTimeKplane
    for name in ("characteristic_loss", "characteristic_loss_at", "characteristic_loss_backward_"):
        assert callable(getattr(TensorVMKeyframeTimeKplane, name, None)), name
    m, meta = make_model("A", device="cpu")
    f = m.nvfi
    ts = float(meta["tmax"]) / (int(meta["num_keyframes"]) - 1)
    assert f.characteristic_time(1.6 * ts) == c64.snap_time(f.num_keyframes, f.tmax, 1.6 * ts)[0]
    assert f.characteristic_time(-1.0) == c64.snap_time(f.num_keyframes, f.tmax, -1.0)[0]
    pts = torch.rand(8, 3) * 2 - 1
    with pytest.raises(_lib.NvfiError):
        f.characteristic_loss(8, ts)
    with pytest.raises(_lib.NvfiError):
        f.characteristic_loss_at(pts, ts)
    with pytest.raises(_lib.NvfiError):
        f.characteristic_loss_backward_(pts, ts)
    m2, _ = make_model("A", device="cpu", use_vel=False)
    with pytest.raises(_lib.NvfiError, match="use_vel"):
        m2.nvfi.characteristic_loss_at(pts, ts)
