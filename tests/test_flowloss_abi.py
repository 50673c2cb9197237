"""The C ABI and the Python surface of the optical-flow loss (nvfi_flow_loss_workspace_bytes, nvfi_flow_loss_fwd, nvfi_flow_loss_bwd;
field.flow_loss), as far as they can be checked without a device: the header declares the three symbols and the built library exports them, every
refusal that is decided on the host before anything is launched, the plan's size, and that tensors without a render behind them are refused."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

TS = 1.0 / 3.0


def _desc(K=4, tmax=1.0, S=64):
    from nvfi_amd import _lib
    d = _lib.FieldDesc()
    d.use_vel, d.K, d.tmax, d.n_samples = 1, K, tmax, S
    return d


def test_header_declares_and_library_exports():
    from nvfi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert re.search(r"int\s+nvfi_flow_loss_workspace_bytes\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t R,\s*float t,\s*float dt,\s*int64_t chunk_cap,\s*int64_t\*\s*bytes\)", hdr)
    assert re.search(r"int\s+nvfi_flow_loss_fwd\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t R,\s*const float\*\s*rays_o,", hdr)
    assert re.search(r"int\s+nvfi_flow_loss_bwd\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t R,\s*float t,\s*float dt,\s*int64_t first,\s*int64_t chunk_cap,", hdr)
    assert "#define NVFI_FLOWLOSS_ADD_GW 1" in hdr and _lib.NVFI_FLOWLOSS_ADD_GW == 1
    assert "#define NVFI_ABI_VERSION 5" in hdr
    L = _lib.lib()
    assert L.nvfi_abi_version() == 5
    for name in ("nvfi_flow_loss_workspace_bytes", "nvfi_flow_loss_fwd", "nvfi_flow_loss_bwd"):
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    # the unit instantiates no MFMA code and stays off the packed-fp32 fence list, as flow.hip and advect.hip do
    from nvfi_amd import build
    assert "flowloss.hip" in build.SOURCES and "flowloss.hip" not in build.NO_PACKED_F32 and "flowloss.hip" not in build.FILE_FLAGS
    src = open(os.path.join(ROOT, "nvfi_amd", "csrc", "flowloss.hip")).read()
    assert "mfma" not in src.lower().replace("no mfma code", "") and "atomicAdd" not in src


def test_workspace_plan():
    from nvfi_amd import _lib
    L = _lib.lib()
    nb = C.c_int64(0)
    d = _desc()

    def plan(R, dt, cap, desc=d, t=0.3):
        rc = L.nvfi_flow_loss_workspace_bytes(C.byref(desc), C.c_int64(R), C.c_float(t), C.c_float(dt), C.c_int64(cap), C.byref(nb))
        return rc

    def adv(N, dt, t=0.3):
        a = C.c_int64(0)
        assert L.nvfi_advect_grad_workspace_bytes(C.byref(d), C.c_int64(N), C.c_float(t), C.c_float(t + dt), C.byref(a)) == 0
        return a.value

    # dt == 0: the per-entry part alone - three float4 images and two times per entry of the R * S capacity, no chunk plan
    assert plan(2048, 0.0, 1000) == 0
    persist = nb.value
    assert 56 * 2048 * 64 <= persist <= 56 * 2048 * 64 + 2048 * 32 + (1 << 20), persist
    assert plan(2048, 0.0, 128) == 0 and nb.value == persist
    # with steps: + the plan of nvfi_advect_grad for chunk_cap points, i.e. the stash size per entry and step tests/test_advect_abi.py pins
    assert plan(2048, TS / 4, 131072) == 0
    one = nb.value
    assert one == persist + adv(131072, TS / 4)
    assert plan(2048, TS / 4 + 3 * TS / 2, 131072) == 0
    per_entry_step = (nb.value - one) / 3 / 131072
    assert 10.5e3 < per_entry_step < 11.1e3, per_entry_step
    assert plan(2048, TS / 4, 128) == 0 and persist + 100e6 < nb.value < persist + 110e6
    # whole 128-entry groups of stash tiles
    assert plan(2048, 0.05, 129) == 0
    a = nb.value
    assert plan(2048, 0.05, 256) == 0 and nb.value - a < 127 * 200
    # 64 steps are planned, 65 refused
    assert plan(4, 31.75 * TS, 128, t=0.0) == 0
    assert plan(4, 32.25 * TS, 128, t=0.0) == 2 and b"more than 64 RK2 steps" in L.nvfi_last_error()
    e = _desc(); e.vel_fp16 = 3
    assert plan(4, 0.1, 128, e) == 0


def _fwd(desc, flags=1, R=4, dt=0.1, pose=1, target=1, ws=None, ws_bytes=0, kind=0, chunk=128, loss_flags=0):
    from nvfi_amd import _lib
    L = _lib.lib()
    p = lambda v: C.c_void_p(v) if v else None       # (fake non-NULL pointers: every call below is refused before anything is launched or read)
    return L.nvfi_flow_loss_fwd(C.byref(desc), C.c_int64(R), p(256), p(256), C.c_float(0.3), C.c_float(dt), C.c_int(flags), p(256),
                                p(256 if pose else 0), 8, 8, C.c_float(10.0), p(256 if target else 0), None, C.c_int(kind), C.c_float(1.0),
                                C.c_float(1.0), None, C.c_int(loss_flags), None, None, None, p(256), C.c_int64(1 << 20), C.c_int64(chunk),
                                p(ws), C.c_int64(ws_bytes), None)


def _bwd(desc, R=4, dt=0.1, first=0, chunk=128, ws=None, ws_bytes=0, grads=True):
    from nvfi_amd import _lib
    L = _lib.lib()
    G = _lib.Grads()
    return L.nvfi_flow_loss_bwd(C.byref(desc), C.c_int64(R), C.c_float(0.3), C.c_float(dt), C.c_int64(first), C.c_int64(chunk),
                                C.byref(G) if grads else None, C.c_void_p(ws) if ws else None, C.c_int64(ws_bytes), None)


def test_every_listed_error_comes_before_a_launch():
    from nvfi_amd import _lib
    L = _lib.lib()
    err = L.nvfi_last_error
    d = _desc()
    assert _fwd(d, flags=0) == 2 and b"NVFI_TRAIN" in err()                    # an eval render: nvfi_render_flow is its branch
    e = _desc(); e.use_vel = 0
    assert _fwd(e) == 2 and b"use_vel" in err() and _bwd(e) == 2
    for mode in (1, 2):
        e = _desc(); e.vel_fp16 = mode
        assert _fwd(e) == 2 and b"vel_fp16" in err() and _bwd(e) == 2
    assert _fwd(d, dt=32.25 * TS) == 2 and b"more than 64 RK2 steps" in err()
    assert _bwd(d, dt=32.25 * TS) == 2 and b"more than 64 RK2 steps" in err()
    assert _fwd(d, pose=0) == 2 and b"pose3x4" in err()
    assert _fwd(d, target=0) == 2 and b"target" in err()
    assert _fwd(d, R=0) == 2 and _fwd(d, kind=2) == 2 and _fwd(d, loss_flags=2) == 2 and _fwd(d, chunk=0) == 2
    assert _bwd(d, first=-1) == 2 and _bwd(d, first=4 * 64) == 2 and _bwd(d, chunk=0) == 2 and _bwd(d, grads=False) == 2
    # error 4: no workspace, a small one, a misaligned one (fake addresses: the size and the alignment are checked before anything is touched)
    nb = C.c_int64(0)
    assert L.nvfi_flow_loss_workspace_bytes(C.byref(d), C.c_int64(4), C.c_float(0.3), C.c_float(0.1), C.c_int64(128), C.byref(nb)) == 0
    assert _fwd(d) == 4 and b"workspace" in err()
    assert _fwd(d, ws=4096, ws_bytes=nb.value - 1) == 4 and b"workspace" in err()
    assert _fwd(d, ws=4096 + 4, ws_bytes=nb.value) == 4 and b"aligned" in err()
    assert _bwd(d) == 4 and _bwd(d, ws=4096, ws_bytes=nb.value - 1) == 4 and _bwd(d, ws=4096 + 8, ws_bytes=nb.value) == 4
    # the error-2 checks come first
    assert _fwd(d, flags=0, ws=4096 + 4, ws_bytes=1) == 2


def test_flow_loss_refuses_foreign_weights():
    from helpers import make_model
    from nvfi_amd import _lib
    model, _ = make_model("A", "cpu")
    f = model.nvfi
    cam = (torch.eye(4)[:3].numpy(), 8, 8, 10.0)
    w = torch.rand(5, f.nSamples, requires_grad=True)
    with pytest.raises(_lib.NvfiError):
        f.flow_loss(w, 0.1, cam, torch.zeros(5, 2))                      # CPU tensors: there is no fallback
    with pytest.raises(_lib.NvfiError):
        model.flow_loss(w * 2.0, 0.1, cam, torch.zeros(5, 2))
    assert hasattr(f, "flow_loss") and hasattr(model, "flow_loss")
    import inspect
    sig = inspect.signature(f.flow_loss)
    assert list(sig.parameters)[:4] == ["weights", "dt", "camera", "target_flow"]
    assert sig.parameters["kind"].default == "l2" and sig.parameters["weight_grad"].default is True and sig.parameters["max_workspace_bytes"].default == 1 << 30
    sig = inspect.signature(f.render_mse_backward_)
    for k, v in dict(target_flow=None, flow_dt=None, flow_camera=None, flow_weight=1.0, flow_valid=None, flow_kind="l2", flow_huber_delta=1.0).items():
        assert sig.parameters[k].default == v, k
