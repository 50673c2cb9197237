"""Differentiable point shading, CPU side: the float64 yardstick (tests/pointshade64.py) against goldens made from the reference's MLPRender_PE /
SHRender under autograd (tests/golden/make_golden_pointshade.py), the ReLU condition of every seed tests/test_gpu_pointshade.py uses, and the
presence of the feature at every layer (header, library, binding, field methods).

Bound of every comparison, per tensor (rgb, g_features, g_xyz, g_view, the six MLP gradients): |got - ref64| <= max(3 x floor, 1e-5 x max |ref64|)
with floor = max |yardstick(float32) - yardstick(float64)| on the same case - lookup64.bound, the rule of tests/test_gpu_pointshade.py.  Measured
here (reference - yardstick / bound): rgb 5e-8 / 5e-6, g_xyz 1.4e-7 / 1.0e-5, g_view 1.5e-7 / 4.8e-6 (A), 3.7e-7 / 3.8e-5 (D), MLP gradients
3e-8 .. 4e-7 / 1e-6 .. 2e-5.  The wrong variants leave the bound by factors of 1e2 and more.

ReLU condition (pointshade64.relu_margin): for every (field, N) below the float64 and the float32 yardstick take the same decision at every hidden
unit (MLP_PE: 256 per point) and at every SH clamp (3 per point), and every pre-activation z has |z64| >= 64 |z32 - z64|.  SEEDS lists the seed of
every case; a seed that missed the condition was replaced by the next one 1000 further that holds it (A: N = 127, 257, 385; B: N = 257, 385; the
first draws were 7000 + N for A and D, 9000 + N for B).  No point is masked out of any comparison."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import point64 as p64
import pointshade64 as s64
from conftest import GOLD, ROOT
from helpers import load_meta

SYMBOLS = ("nvfi_render_mlp_grad_workspace_bytes", "nvfi_render_mlp_grad")
KINDS = ("A", "B", "D")
SIZES = (1, 31, 32, 33, 127, 128, 129, 257)       # the raw cases of the GPU file: wave-tile (32) and workgroup (128) edges
CHUNK_N = 385                                     # its chunked case: four 128-point chunks
# (field, N) -> seed of pointshade64.inputs.  B shares A's render MLP (make_golden.py), so it draws other inputs
SEEDS = {("A", 1): 7001, ("A", 31): 7031, ("A", 32): 7032, ("A", 33): 7033, ("A", 127): 8127, ("A", 128): 7128, ("A", 129): 7129, ("A", 257): 11257,
         ("A", 385): 8385,
         ("B", 1): 9001, ("B", 31): 9031, ("B", 32): 9032, ("B", 33): 9033, ("B", 127): 9127, ("B", 128): 9128, ("B", 129): 9129, ("B", 257): 13257,
         ("B", 385): 10385,
         ("D", 1): 7001, ("D", 31): 7031, ("D", 32): 7032, ("D", 33): 7033, ("D", 127): 7127, ("D", 128): 7128, ("D", 129): 7129, ("D", 257): 7257,
         ("D", 385): 7385}
_cache = {}


@pytest.fixture(scope="module")
def sg():
    return np.load(os.path.join(GOLD, "pointshade.npz"))


def golden_field(kind):
    """A, B (A's render MLP) and D: A with SH shading - SHRender has no parameters"""
    if kind not in _cache:
        meta, sd = load_meta("A" if kind == "D" else kind)
        if kind == "B":
            for k, v in load_meta("A")[1].items():
                sd.setdefault(k, v)
        _cache[kind] = p64.field_of(sd, meta, sh=kind == "D")
    return _cache[kind]


def yardsticks(sg, kind):
    """(float64, float32, wrong float64) results of a golden case, computed once"""
    key = (kind, "y")
    if key not in _cache:
        a = [sg[f"{kind}:{k}"] for k in ("xyz", "view", "feat", "g")]
        f = golden_field(kind)
        _cache[key] = (s64.shade64(f, *a), s64.shade64(f, *a, dtype=torch.float32), s64.shade64(f, *a, wrong=True))
    return _cache[key]


def golden_tensors(sg, kind):
    return {k[2:]: sg[k] for k in sg.files if k.startswith(kind + ":") and k[2:] not in ("xyz", "view", "feat", "g")}


@pytest.mark.parametrize("kind", KINDS)
def test_yardstick_reproduces_reference_goldens(sg, kind):
    y64, y32, _ = yardsticks(sg, kind)
    t64, t32, ref = s64.tensors(y64), s64.tensors(y32), golden_tensors(sg, kind)
    assert set(t64) == set(ref) and len(t64) == (4 if kind == "D" else 10)
    assert sg[f"{kind}:xyz"].shape[0] <= 64
    for label in t64:
        e, b = s64.max_err(ref[label], t64[label]), s64.bound(t64[label], t32[label])
        print(f"{kind}:{label}: reference - yardstick {e:.2e}, float32 floor {s64.max_err(t32[label], t64[label]):.2e}, bound {b:.2e}")
        if not (kind == "D" and label == "g_xyz"):
            assert np.abs(t64[label]).max() > 0, (kind, label, "nothing to compare")
        assert e <= b, (kind, label, e, b)
    if kind == "D":
        assert not ref["g_xyz"].any() and not t64["g_xyz"].any(), "SHRender does not read xyz"


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_variant_is_outside_the_bound(sg, kind):
    """MLP_PE: the view encoding's top frequency dropped - the colour, g_view and mlp.0.weight's gradient move; SH: b[6] without its factor 2"""
    y64, y32, bad = yardsticks(sg, kind)
    t64, t32, tb, ref = s64.tensors(y64), s64.tensors(y32), s64.tensors(bad), golden_tensors(sg, kind)
    labels = ["rgb", "g_view"] + ([] if kind == "D" else ["grad:renderModule.mlp.0.weight"])
    for label in labels:
        e, b = s64.max_err(ref[label], tb[label]), s64.bound(t64[label], t32[label])
        print(f"{kind}:{label}: reference - wrong variant {e:.2e}, bound {b:.2e}")
        assert e > 3 * b, (kind, label, e, b)


@pytest.mark.parametrize("kind", KINDS)
def test_relu_condition_of_every_gpu_seed(sg, kind):
    f = golden_field(kind)
    cases = [(N, SEEDS[(kind, N)]) for N in SIZES + (CHUNK_N,)]
    assert len(SEEDS) == 3 * (len(SIZES) + 1)
    for N, seed in cases:
        xyz, view, feat, _ = s64.inputs(f, N, seed)
        same, room = s64.relu_margin(f, xyz, view, feat)
        print(f"{kind}: N={N} seed={seed}: same decisions {same}, smallest |z64| / (64 |z32 - z64|) = {room:.2f}")
        assert same and room >= 1.0, (kind, N, seed, same, room)
    same, room = s64.relu_margin(f, sg[f"{kind}:xyz"], sg[f"{kind}:view"], sg[f"{kind}:feat"])
    assert same and room >= 1.0, (kind, "golden", same, room)


def test_header_library_and_binding():
    from nvfi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    assert re.search(r"#define NVFI_ABI_VERSION 5\b", hdr)
    assert re.search(r"int\s+nvfi_render_mlp_grad_workspace_bytes\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*int64_t\*\s*bytes\)\s*;", hdr)
    assert re.search(r"int\s+nvfi_render_mlp_grad\s*\(\s*const nvfi_field_desc\*\s*f,\s*int64_t N,\s*const float\*\s*xyz.*?const float\*\s*view.*?const float\*\s*features"
                     r".*?const float\*\s*g_rgb.*?float\*\s*g_features.*?float\*\s*g_xyz.*?float\*\s*g_view.*?const nvfi_grads\*\s*grads.*?void\*\s*workspace,"
                     r"\s*int64_t workspace_bytes,\s*void\*\s*stream\)\s*;", hdr, re.S)
    assert os.path.exists(_lib.SO), "libnvfi_hip.so has not been built"
    L = C.CDLL(_lib.SO)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.nvfi_abi_version() == 5
    from nvfi_amd.build import SOURCES
    assert "point_shade.hip" in SOURCES
    from nvfi_amd.utils import field_lookup as fl
    assert callable(fl.render_mlp_grad_raw)


def test_refused_before_anything_is_launched():
    """error 2 (descriptor, N >= 2^31 - 256, a NULL input) and error 4 (workspace under the published size) come before the first HIP call: this
    runs without a GPU, on a host-built descriptor and dummy pointers that nothing may dereference; an empty call is a no-op"""
    from nvfi_amd import _lib
    from test_abi_and_host import _plan_desc
    L = _lib.lib()
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)
    G = _lib.Grads()
    big = C.c_int64(1 << 40)

    def call(d, n, ptrs=(p, p, p, p), ws=p, ws_bytes=big):
        return L.nvfi_render_mlp_grad(C.byref(d), C.c_int64(n), *ptrs, p, p, p, C.byref(G), ws, ws_bytes, None)

    def refused(rc, code, *words):
        msg = L.nvfi_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    d = _plan_desc()
    nb = C.c_int64(0)
    for n in ((1 << 31) - 256, 1 << 31, 1 << 40):
        refused(call(d, n), 2, "nvfi_render_mlp_grad", "N too large")
        refused(L.nvfi_render_mlp_grad_workspace_bytes(C.byref(d), C.c_int64(n), C.byref(nb)), 2, "N too large")
    assert call(d, 0) == 0 and call(d, -3) == 0
    for k in range(4):
        refused(call(d, 16, ptrs=tuple(None if j == k else p for j in range(4))), 2, "non-NULL")
    need = _lib.bytes_of(L.nvfi_render_mlp_grad_workspace_bytes, C.byref(d), C.c_int64(16))
    # counted: 16 count words, the fragments, 2 x 16 B per point, four stash tiles (one workgroup) of 224 + 160 rows and 1 KB of masks, 3 slab sets
    frag = 4 * (1 * 24 * 64 + 4 * 55 * 64 + 4 * 64 * 64 + 1 * 64 * 64 + 128 + 128 + 32 + 4 * 4 * 64 + 2 * 4 * 64 * 64 + 2 * 16 * 64)
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    counted = up(64) + up(frag) + 2 * up(16 * 16) + up(4 * 224 * 256) + up(4 * 160 * 256) + up(4 * 1024) + up(3 * 256 * (128 * 128 + 128) * 4)
    assert need == counted, (need, counted)
    refused(call(d, 16, ws_bytes=C.c_int64(need - 1)), 4, "workspace too small")
    refused(call(d, 16, ws=None), 4, "workspace too small")
    assert _lib.bytes_of(L.nvfi_render_mlp_grad_workspace_bytes, C.byref(d), C.c_int64(129)) - need == 2 * (up(129 * 16) - up(256)) + 4 * (224 + 160 + 4) * 256
    d.Cd = 16
    refused(call(d, 16), 2, "Cd=16")
    refused(call(d, 0), 2, "Cd=16")            # the descriptor is checked before the empty call returns 0
    assert not any(dummy), "a refused call wrote through its pointers"


def test_field_methods_exist_and_refuse_the_cpu():
    from helpers import make_model
    from nvfi_amd import _lib
    from nvfi_amd.models import NVFi
    from nvfi_amd.models.field_autograd import _ShadeFn
    from nvfi_amd.models.tensorf_keyframe import TensorVMKeyframeTimeKplane
    assert _ShadeFn.N_ARGS == 5
    for cls in (TensorVMKeyframeTimeKplane, NVFi):
        for name in ("shade", "lookup_rgb"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    m, _ = make_model("A", device="cpu")
    q, v, fe = torch.rand(8, 4) * 2 - 1, torch.randn(8, 3), torch.randn(8, 32)
    for obj in (m.nvfi, m):
        with pytest.raises(_lib.NvfiError):
            obj.shade(q[:, :3], v, fe)
        with pytest.raises(_lib.NvfiError):
            obj.shade(q[:, :3], v, fe.clone().requires_grad_(True))
        with pytest.raises(_lib.NvfiError):
            obj.lookup_rgb(q, v)
