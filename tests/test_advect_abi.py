"""The C ABI and the Python surface of differentiable advection (nvfi_advect_grad_workspace_bytes, nvfi_advect_grad; field.advect), as far as they
can be checked without a device: the header declares the two symbols and the built library exports them, the refusals that are decided on the host
before anything is launched, the plan's size, and that CPU tensors are refused (there is no fallback)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT


def _desc(K=4, tmax=1.0):
    from nvfi_amd import _lib
    d = _lib.FieldDesc()
    d.use_vel, d.K, d.tmax = 1, K, tmax
    return d


def test_header_declares_and_library_exports():
    from nvfi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert re.search(r"int\s+nvfi_advect_grad_workspace_bytes\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*float t,\s*float t_target,\s*int64_t\*\s*bytes\)", hdr)
    assert re.search(r"int\s+nvfi_advect_grad\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*x,\s*float t,\s*float t_target,", hdr)
    assert "#define NVFI_ABI_VERSION 5" in hdr
    L = _lib.lib()
    assert L.nvfi_abi_version() == 5
    for name in ("nvfi_advect_grad_workspace_bytes", "nvfi_advect_grad"):
        assert name in _lib.EXPORTS and getattr(L, name) is not None


def test_host_side_refusals_and_plan():
    from nvfi_amd import _lib
    L = _lib.lib()
    nb = C.c_int64(0)
    d = _desc()
    ts = 1.0 / 3.0

    def plan(N, t, t1, desc=d):
        return L.nvfi_advect_grad_workspace_bytes(C.byref(desc), C.c_int64(N), C.c_float(t), C.c_float(t1), C.byref(nb))

    def grad(N, t, t1, desc=d):
        return L.nvfi_advect_grad(C.byref(desc), C.c_int64(N), None, C.c_float(t), C.c_float(t1), None, None, None, None, C.c_int64(0), C.c_void_p(0))
    # 64 steps (63 of ts / 2 and a remainder) are planned, 65 are refused with error 2 (not truncated) by both calls
    assert plan(128, 0.0, 31.75 * ts) == 0 and nb.value > 0
    assert plan(128, 0.0, 32.25 * ts) == 2 and b"more than 64 RK2 steps" in L.nvfi_last_error()
    assert grad(128, 0.0, 32.25 * ts) == 2 and b"more than 64 RK2 steps" in L.nvfi_last_error()
    assert grad(0, 0.0, 32.25 * ts) == 2                       # (the schedule is checked before the size)
    # nothing to do: N == 0 returns 0 without touching a pointer; t == t_target plans the minimum
    assert grad(0, 0.3, 0.4) == 0
    assert plan(1000, 0.3, 0.3) == 0 and nb.value == 256
    # the stash: (VEL_Z_REGS + VEL_X0_REGS + VEL_G_REGS) * 64 * 4 B per 32-point tile and evaluation, two evaluations per step, + the 19-float
    # record - about 10.8 KB per point and step - and 101 MB of slabs; 262 144 points at one step are 2.8 GB
    assert plan(262144, 0.3, 0.3 + ts / 4) == 0
    one = nb.value
    assert 2.7e9 < one < 3.1e9, one
    assert plan(262144, 0.3, 0.3 + ts / 4 + 3 * ts / 2) == 0
    per_point_step = (nb.value - one) / 3 / 262144
    assert 10.5e3 < per_point_step < 11.1e3, per_point_step
    assert plan(128, 0.3, 0.3 + ts / 4) == 0 and 100e6 < nb.value < 110e6
    # whole 128-point groups of stash tiles
    assert plan(129, 0.3, 0.35) == 0
    a = nb.value
    assert plan(256, 0.3, 0.35) == 0 and nb.value - a < 127 * 200
    # no velocity net, fp16-input modes: error 2
    e = _desc(); e.use_vel = 0
    assert plan(128, 0.3, 0.4, e) == 2 and b"use_vel" in L.nvfi_last_error()
    for mode in (1, 2):
        e = _desc(); e.vel_fp16 = mode
        assert plan(128, 0.3, 0.4, e) == 2 and grad(128, 0.3, 0.4, e) == 2 and b"vel_fp16" in L.nvfi_last_error()
    e = _desc(); e.vel_fp16 = 3
    assert plan(128, 0.3, 0.4, e) == 0


def test_advect_refuses_cpu_tensors():
    from helpers import make_model
    from nvfi_amd import _lib
    model, _ = make_model("A", "cpu")
    x = torch.zeros(5, 3, requires_grad=True)
    with pytest.raises(_lib.NvfiError):
        model.nvfi.advect(x, 0.3, 0.4)
    with pytest.raises(_lib.NvfiError):
        model.advect(x.detach(), 0.3, 0.4)
    with torch.no_grad(), pytest.raises(_lib.NvfiError):
        model.advect(x, 0.3, 0.3)
