"""The C ABI and the Python surface of differentiable advection with per-point times (nvfi_advect_pt_steps, nvfi_advect_grad_pt_workspace_bytes,
nvfi_advect_grad_pt; field.advect_pt), as far as they can be checked without a device: the header declares the three symbols (include/nvfi_hip_advect_pt.h,
brought in by nvfi_hip.h) and the built library exports them, the rows of the binding's table, every refusal that is decided on the host before
anything is launched, the plan's size, the chunk plan of the backward, and that CPU tensors and time tensors that require grad are refused."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

TS = 1.0 / 3.0
NAMES = ("nvfi_advect_pt_steps", "nvfi_advect_grad_pt_workspace_bytes", "nvfi_advect_grad_pt")


def _desc(K=4, tmax=1.0):
    from nvfi_amd import _lib
    d = _lib.FieldDesc()
    d.use_vel, d.K, d.tmax = 1, K, tmax
    return d


def _prototypes(text):
    """[(name, return type, kinds)] of the prototypes in a header's text, by the rule of tests/test_abi_and_host.py: comments and preprocessor
    lines stripped, a letter per parameter - p for anything with a `*`, l int64_t, i int, f float"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(nvfi_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(q.split()) for q in params.split(",")]
        out.append((name, " ".join(ret.split()), "".join("p" if "*" in q else {"int64_t": "l", "int": "i", "float": "f"}[q.rsplit(" ", 1)[0]] for q in params)))
    return out


def test_header_declares_and_library_exports():
    """the three prototypes stand in include/nvfi_hip_advect_pt.h, which include/nvfi_hip.h brings in behind nvfi_advect_grad (so a C consumer
    of nvfi_hip.h sees them); their rows are _lib.ADDITIONS["nvfi_hip_advect_pt.h"], bound by lib() like the rows of SIGNATURES"""
    from nvfi_amd import _lib, build
    main = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip_advect_pt.h")).read()
    inc = main.index('#include "nvfi_hip_advect_pt.h"')
    assert main.index("int nvfi_advect_grad(") < inc < main.index("int nvfi_density_at(") and inc < main.rindex("#ifdef __cplusplus")
    assert "#define NVFI_ABI_VERSION 5" in main and "NVFI_ABI_VERSION" not in hdr
    assert re.search(r"int\s+nvfi_advect_pt_steps\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*t,\s*const float\*\s*t_target,\s*"
                     r"int32_t\*\s*steps,\s*int64_t\*\s*hist66,\s*void\*\s*stream\)", hdr)
    assert re.search(r"int\s+nvfi_advect_grad_pt_workspace_bytes\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*int max_steps,\s*int64_t\*\s*bytes\)", hdr)
    assert re.search(r"int\s+nvfi_advect_grad_pt\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*x,\s*const float\*\s*t,\s*"
                     r"const float\*\s*t_target,\s*int max_steps,", hdr)
    protos = _prototypes(hdr)
    rows = _lib.ADDITIONS["nvfi_hip_advect_pt.h"]
    assert [n for n, _, _ in protos] == list(NAMES) == list(rows) and not set(rows) & set(_lib.SIGNATURES)
    L = _lib.lib()
    assert L.nvfi_abi_version() == 5
    for name, ret, kinds in protos:
        fn = getattr(L, name)
        assert ret == "int" and rows[name] == kinds and list(fn.argtypes) == [_lib.KINDS[k] for k in kinds] and fn.restype is C.c_int, name
    assert rows == {"nvfi_advect_pt_steps": "plppppp", "nvfi_advect_grad_pt_workspace_bytes": "plip", "nvfi_advect_grad_pt": "plpppippppplp"}
    # the build knows the header; the unit is host code and two small kernels: no MFMA code, off the packed-fp32 fence list, and the one step
    # loop is common.h's
    assert any(h.endswith("nvfi_hip_advect_pt.h") for h in build.HEADERS)
    assert "advect_pt.hip" in build.SOURCES and "advect_pt.hip" not in build.NO_PACKED_F32 and "advect_pt.hip" not in build.FILE_FLAGS
    src = open(os.path.join(ROOT, "nvfi_amd", "csrc", "advect_pt.hip")).read()
    assert "mfma" not in src.lower() and src.count("rk_steps(dtm,") == 2 and "while" not in re.sub(r"//[^\n]*", "", src)


def _plan(d, N, ms):
    from nvfi_amd import _lib
    nb = C.c_int64(0)
    rc = _lib.lib().nvfi_advect_grad_pt_workspace_bytes(C.byref(d), N, ms, C.byref(nb))
    return rc, nb.value


def test_workspace_plan():
    from nvfi_amd import _lib
    L = _lib.lib()
    d = _desc()

    def adv(N, dt, t=0.3):
        a = C.c_int64(0)
        assert L.nvfi_advect_grad_workspace_bytes(C.byref(d), N, t, t + dt, C.byref(a)) == 0
        return a.value

    def table(N, ms):
        return (8 * N * ms + 255) // 256 * 256

    # nvfi_advect_grad's plan at the same step count, plus the table: 8 bytes per point and step
    for N, dt, ms in ((128, TS / 4, 1), (129, TS / 4, 1), (131072, TS / 4, 1), (131072, TS / 4 + 3 * TS / 2, 4), (257, 31.75 * TS, 64)):
        rc, nb = _plan(d, N, ms)
        assert rc == 0 and nb == adv(N, dt, t=0.0 if ms == 64 else 0.3) + table(N, ms), (N, ms, nb)
    # it grows with N * max_steps: ~10.8 KB of stash per point and step, as nvfi_advect_grad's
    one, four = _plan(d, 131072, 1)[1], _plan(d, 131072, 4)[1]
    assert 10.5e3 < (four - one) / 3 / 131072 < 11.1e3
    assert _plan(d, 262144, 4)[1] - four > 0.99 * (four - _plan(d, 128, 4)[1])
    # whole 128-point groups of stash tiles
    assert _plan(d, 256, 2)[1] - _plan(d, 129, 2)[1] < 127 * 400
    # nothing to do: the token size
    assert _plan(d, 0, 4) == (0, 256) and _plan(d, 1000, 0) == (0, 256)
    e = _desc(); e.vel_fp16 = 3
    assert _plan(e, 128, 4)[0] == 0


def _grad(d, N=4, ms=2, ws=None, ws_bytes=0, x=256, t=256, t1=256, g=256, grads=True):
    from nvfi_amd import _lib
    G = _lib.Grads()
    p = lambda v: C.c_void_p(v) if v else None       # (fake non-NULL pointers: every call below is refused before anything is launched or read)
    return _lib.lib().nvfi_advect_grad_pt(C.byref(d), N, p(x), p(t), p(t1), ms, p(g), None, C.byref(G) if grads else None, None, p(ws), ws_bytes, None)


def test_every_listed_error_comes_before_a_launch():
    from nvfi_amd import _lib
    L = _lib.lib()
    err = L.nvfi_last_error
    d = _desc()
    assert _grad(d, N=-1) == 2 and _plan(d, -1, 2)[0] == 2
    assert _grad(d, N=(1 << 31) - 256) == 2 and b"too large" in err() and _plan(d, (1 << 31) - 256, 2)[0] == 2
    e = _desc(); e.use_vel = 0
    assert _grad(e) == 2 and b"use_vel" in err() and _plan(e, 4, 2)[0] == 2
    assert L.nvfi_advect_pt_steps(C.byref(e), 4, C.c_void_p(256), C.c_void_p(256), None, C.c_void_p(256), None) == 2 and b"use_vel" in err()
    assert L.nvfi_advect_pt_steps(C.byref(d), -1, C.c_void_p(256), C.c_void_p(256), None, C.c_void_p(256), None) == 2
    assert L.nvfi_advect_pt_steps(C.byref(d), 4, C.c_void_p(256), C.c_void_p(256), None, None, None) == 2 and b"hist66" in err()
    for mode in (1, 2):
        e = _desc(); e.vel_fp16 = mode
        assert _grad(e) == 2 and b"vel_fp16" in err() and _plan(e, 4, 2)[0] == 2
    for ms in (-1, 65):
        assert _grad(d, ms=ms) == 2 and b"max_steps" in err() and _plan(d, 4, ms)[0] == 2
    assert _plan(d, 4, 64)[0] == 0
    assert _grad(d, g=0) == 2 and b"g_xk" in err()
    assert _grad(d, x=0) == 2 and _grad(d, t=0) == 2 and _grad(d, t1=0) == 2 and _grad(d, grads=False) == 2
    # error 4: no workspace, one byte short (a fake address: the size is checked before anything is touched)
    nb = _plan(d, 4, 2)[1]
    assert _grad(d) == 4 and b"workspace" in err()
    assert _grad(d, ws=4096, ws_bytes=nb - 1) == 4 and b"workspace" in err()
    # the error-2 checks come first
    assert _grad(d, ms=65, ws=4096, ws_bytes=1) == 2
    # N == 0: nothing to do, nothing launched
    assert _grad(d, N=0) == 0


def test_chunk_plan_follows_the_steps():
    """_AdvectPtFn.plan: one plan_chunks per step count that occurs, largest first, every chunk under the budget with its own max_steps, the
    zero-step points last as one entry that launches nothing"""
    from nvfi_amd import _lib
    from nvfi_amd.models.field_autograd import _AdvectPtFn
    d = _desc()
    nbytes = lambda n, s: _plan(d, n, s)[1]
    hist = [0] * 65
    hist[0], hist[1], hist[3], hist[8] = 52, 51, 51, 300
    chunks, ws = _AdvectPtFn.plan(nbytes, hist, 1 << 30)
    assert chunks == [(0, 300, 8), (300, 51, 3), (351, 51, 1), (402, 52, 0)] and ws == nbytes(300, 8)
    budget = nbytes(128, 8) + 4096
    chunks, ws = _AdvectPtFn.plan(nbytes, hist, budget)
    assert [c[2] for c in chunks] == sorted((c[2] for c in chunks), reverse=True) and chunks[-1] == (402, 52, 0)
    assert sum(c[1] for c in chunks) == 454 and [c[0] for c in chunks] == [sum(c[1] for c in chunks[:k]) for k in range(len(chunks))]
    assert all(nbytes(n, s) <= budget for _, n, s in chunks if s) and ws <= budget
    assert [c[1] for c in chunks if c[2] == 8] == [128, 128, 44] and [c[1] for c in chunks if c[2] in (3, 1)] == [51, 51]
    with pytest.raises(_lib.NvfiError):
        _AdvectPtFn.plan(nbytes, hist, nbytes(128, 8) - 1)
    assert _AdvectPtFn.plan(nbytes, [7] + [0] * 64, 1 << 30) == ([(0, 7, 0)], 0)


def test_advect_pt_refuses_cpu_tensors_and_times_with_grad():
    from helpers import make_model
    from nvfi_amd import _lib
    model, _ = make_model("A", "cpu")
    f = model.nvfi
    x = torch.rand(5, 3, requires_grad=True)
    t = torch.rand(5)
    with pytest.raises(_lib.NvfiError, match="GPU"):
        f.advect_pt(x, t, t + 0.1)                                      # CPU tensors: there is no fallback
    with pytest.raises(_lib.NvfiError, match="GPU"):
        model.advect_pt(x, 0.1, 0.2)
    tg = t.clone().requires_grad_(True)
    with pytest.raises(_lib.NvfiError, match="requires grad"):
        f.advect_pt(x, tg, t + 0.1)
    with pytest.raises(_lib.NvfiError, match="requires grad"):
        f.advect_pt(x, t, tg + 0.1)
    import inspect
    sig = inspect.signature(f.advect_pt)
    assert list(sig.parameters) == ["pos", "t", "t_target", "max_workspace_bytes"] and sig.parameters["max_workspace_bytes"].default == 1 << 30
    assert list(inspect.signature(model.advect_pt).parameters) == ["pos", "t", "t_target", "max_workspace_bytes"]
