"""The C ABI and the Python surface of the mask loss (nvfi_mask_loss_workspace_bytes, nvfi_mask_loss_fwd, nvfi_mask_loss_bwd; field.mask_loss,
field.mask_fit_backward_, render_mse_backward_(target_mask=)), as far as they can be checked without a device: the header declares the three
symbols and the built library exports them, the plan's size, every refusal that is decided on the host before anything is launched, and that
tensors without a render behind them are refused."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def _desc(S=64):
    from nvfi_amd import _lib
    d = _lib.FieldDesc()
    d.use_vel, d.K, d.tmax, d.n_samples = 1, 4, 1.0, S
    return d


def _mdesc(K=8, n_layer=4, n_dim=128, ptrs=True):
    from nvfi_amd import _lib
    m = _lib.MaskDesc()
    m.n_layer, m.n_dim, m.mask_dim = n_layer, n_dim, K
    for i in range(5):      # (fake non-NULL pointers: nothing below gets as far as reading them)
        m.W[i] = 256 if ptrs else None
        m.b[i] = 256 if ptrs else None
    return m


def test_header_declares_and_library_exports():
    from nvfi_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert re.search(r"int\s+nvfi_mask_loss_workspace_bytes\s*\(\s*const nvfi_field_desc\*\s*f,\s*const nvfi_mask_desc\*\s*m,\s*int64_t R,\s*int64_t chunk_cap,\s*int64_t\*\s*bytes\)", hdr)
    assert re.search(r"int\s+nvfi_mask_loss_fwd\s*\(\s*const nvfi_field_desc\*\s*f,\s*const nvfi_mask_desc\*\s*m,\s*int64_t R,\s*float t,\s*int flags,", hdr)
    assert re.search(r"int\s+nvfi_mask_loss_bwd\s*\(\s*const nvfi_mask_desc\*\s*m,\s*int64_t R,\s*int S,\s*int64_t first,\s*int64_t chunk_cap,", hdr)
    assert "#define NVFI_MASKLOSS_ADD_GW 1" in hdr and _lib.NVFI_MASKLOSS_ADD_GW == 1
    assert "#define NVFI_ABI_VERSION 5" in hdr
    L = _lib.lib()
    assert L.nvfi_abi_version() == 5
    for name in ("nvfi_mask_loss_workspace_bytes", "nvfi_mask_loss_fwd", "nvfi_mask_loss_bwd"):
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    # fp32 MFMA only: no 16-bit matrix instruction, so the unit stays off the packed-fp32 fence list; every clear is a kernel
    assert "maskloss.hip" in build.SOURCES and "maskloss.hip" not in build.NO_PACKED_F32 and "maskloss.hip" not in build.FILE_FLAGS
    src = open(os.path.join(ROOT, "nvfi_amd", "csrc", "maskloss.hip")).read()
    assert "MFMA16" not in src and "engine16.h" not in src and "hipMemset" not in src and "atomicAdd" not in src
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src


def _plan(R, cap, d=None, m=None):
    from nvfi_amd import _lib
    nb = C.c_int64(-1)
    rc = _lib.lib().nvfi_mask_loss_workspace_bytes(C.byref(d or _desc()), C.byref(m or _mdesc()), C.c_int64(R), C.c_int64(cap), C.byref(nb))
    return rc, nb.value


def test_workspace_plan():
    sizes = {}
    for R in (1, 2, 33, 257, 2048):
        for cap in (128, 256, 1024, 8192):
            rc, sizes[R, cap] = _plan(R, cap)
            assert rc == 0 and sizes[R, cap] % 256 == 0
    # monotone in R and in chunk_cap
    for cap in (128, 256, 1024, 8192):
        col = [sizes[R, cap] for R in (1, 2, 33, 257, 2048)]
        assert col == sorted(col) and len(set(col)) == len(col), col
    for R in (1, 2, 33, 257, 2048):
        row = [sizes[R, cap] for cap in (128, 256, 1024, 8192)]
        assert row == sorted(row) and len(set(row)) == len(row), row
    # per entry of the capacity: a float4 (position, weight), the ray index and 32 softmax floats = 148 bytes; per ray 32 g_q floats, a double, a flag
    S = 64
    per_entry = (sizes[2048, 128] - sizes[257, 128]) / ((2048 - 257) * S)
    assert 148 <= per_entry <= 148 + (128 + 12) / S + 0.1, per_entry
    # per entry of a chunk: the forward stash (288 rows), the adjoint stash (272 rows), 64 floats each per 32 entries, + the ReLU sign words
    per_chunk_entry = (sizes[33, 8192] - sizes[33, 1024]) / (8192 - 1024)
    assert per_chunk_entry == (288 + 272) * 64 * 4 / 32 + 512 * 4 / 32, per_chunk_entry
    # the five slab sets of the weight-gradient jobs do not grow with either
    slabs = 5 * 256 * (128 * 128 + 128) * 4
    assert slabs < sizes[1, 128] < slabs + (1 << 20)
    # K does not move the plan (the softmax rows are 32 wide for every K)
    assert _plan(33, 1024, m=_mdesc(K=32))[1] == sizes[33, 1024] == _plan(33, 1024, m=_mdesc(K=1))[1]


def _fwd(d=None, m=None, R=4, flags=1, labels=1, soft=0, kind=1, eps=1e-5, loss_flags=0, gw=0, chunk=128, ws=None, ws_bytes=0, weights=1, rws=1):
    from nvfi_amd import _lib
    p = lambda v: C.c_void_p(v) if v else None       # (fake non-NULL pointers: every call below is refused before anything is launched or read)
    return _lib.lib().nvfi_mask_loss_fwd(C.byref(d or _desc()), C.byref(m or _mdesc()), C.c_int64(R), C.c_float(0.3), C.c_int(flags), p(256 * weights),
                                         p(256 * labels), p(256 * soft), C.c_int(kind), C.c_float(eps), C.c_float(1.0), None, C.c_int(loss_flags),
                                         None, None, p(256 * gw), p(256 * rws), C.c_int64(1 << 20), C.c_int64(chunk), p(ws), C.c_int64(ws_bytes), None)


def _bwd(m=None, R=4, S=64, first=0, chunk=128, ws=None, ws_bytes=0, grads=True):
    from nvfi_amd import _lib
    G = _lib.MaskGrads()
    return _lib.lib().nvfi_mask_loss_bwd(C.byref(m or _mdesc()), C.c_int64(R), C.c_int(S), C.c_int64(first), C.c_int64(chunk),
                                         C.byref(G) if grads else None, C.c_void_p(ws) if ws else None, C.c_int64(ws_bytes), None)


def test_every_listed_error_comes_before_a_launch():
    from nvfi_amd import _lib
    err = _lib.lib().nvfi_last_error
    # a mask desc that mask_check refuses
    for bad in (_mdesc(K=0), _mdesc(K=33), _mdesc(n_layer=3), _mdesc(n_dim=64), _mdesc(ptrs=False)):
        assert _fwd(m=bad) == 2 and b"mask field" in err()
        assert _bwd(m=bad) == 2 and _plan(4, 128, m=bad)[0] == 2
    assert _fwd(R=0) == 2 and b"R=0" in err() and _bwd(R=0) == 2 and _plan(0, 128)[0] == 2
    assert _fwd(labels=1, soft=1) == 2 and b"exactly one" in err()
    assert _fwd(labels=0, soft=0) == 2 and b"exactly one" in err()
    assert _fwd(labels=0, soft=1, ws=None) == 4                       # soft alone is a valid choice: the next refusal is the workspace's
    assert _fwd(kind=2) == 2 and _fwd(kind=-1) == 2 and b"kind" in err()
    assert _fwd(loss_flags=2) == 2 and b"loss_flags" in err()
    assert _fwd(loss_flags=1, gw=0) == 2                                # nothing to add to
    assert _fwd(kind=1, eps=0.0) == 2 and b"eps" in err() and _fwd(kind=1, eps=-1.0) == 2
    assert _fwd(kind=0, eps=0.0) == 4                                   # l2 does not read eps
    for chunk in (0, -128, 127, 129, 192):
        assert _fwd(chunk=chunk) == 2 and b"chunk_cap" in err(), chunk
        assert _bwd(chunk=chunk) == 2 and _plan(4, chunk)[0] == 2
    assert _bwd(first=-128) == 2 and _bwd(first=4 * 64) == 2 and _bwd(first=64) == 2 and _bwd(grads=False) == 2
    # error 4: no workspace, a small one, a misaligned one (fake addresses: the size and the alignment are checked before anything is touched)
    rc, nb = _plan(4, 128)
    assert rc == 0
    assert _fwd() == 4 and b"workspace" in err()
    assert _fwd(ws=4096, ws_bytes=nb - 1) == 4 and b"workspace" in err()
    assert _fwd(ws=4096 + 4, ws_bytes=nb) == 4 and b"aligned" in err()
    assert _bwd() == 4 and _bwd(ws=4096, ws_bytes=nb - 1) == 4 and _bwd(ws=4096 + 8, ws_bytes=nb) == 4
    # the error-2 checks come first
    assert _fwd(kind=2, ws=4096 + 4, ws_bytes=1) == 2


def test_python_surface_and_refusals():
    from helpers import make_model
    from nvfi_amd import _lib
    from nvfi_amd.models import MaskField
    from nvfi_amd.utils import mask_loss as ml
    model, _ = make_model("A", "cpu")
    f = model.nvfi
    mf = MaskField(mask_dim=8)
    w = torch.rand(5, f.nSamples, requires_grad=True)
    with pytest.raises(ValueError):
        f.mask_loss(w, torch.zeros(5, dtype=torch.int64))                # no mask field anywhere
    with pytest.raises(_lib.NvfiError):
        f.mask_loss(w, torch.zeros(5, dtype=torch.int64), mask_field=mf)  # CPU tensors: there is no fallback
    with pytest.raises(_lib.NvfiError):
        model.mask_loss(w * 2.0, torch.zeros(5, dtype=torch.int64), mask_field=mf)
    with pytest.raises(NotImplementedError):
        f.mask_loss(w, torch.zeros(5, dtype=torch.int64), mask_field=MaskField(mask_dim=8, mfma_fp16=True))
    sig = inspect.signature(f.mask_loss)
    assert list(sig.parameters)[:3] == ["weights", "target", "mask_field"]
    for k, v in dict(mask_field=None, kind="ce", eps=1e-5, weight_grad=True, max_workspace_bytes=1 << 30).items():
        assert sig.parameters[k].default == v, k
    sig = inspect.signature(f.render_mse_backward_)
    for k, v in dict(target_mask=None, mask_field=None, mask_weight=1.0, mask_kind="ce", mask_eps=1e-5, mask_max_workspace_bytes=1 << 30).items():
        assert sig.parameters[k].default == v, k
    sig = inspect.signature(f.mask_fit_backward_)
    assert list(sig.parameters)[:4] == ["t", "ray_o", "ray_d", "target_mask"]
    for k, v in dict(mask_field=None, kind="ce", eps=1e-5, loss_scale=1.0, white_bg=True, jitter=None).items():
        assert sig.parameters[k].default == v, k
    assert ml.KINDS == {"l2": 0, "ce": 1}
    for name in ("mask_loss_plan", "mask_loss_raw", "mask_loss_backward_raw"):
        assert callable(getattr(ml, name))
