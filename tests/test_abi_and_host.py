"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol the header declares, the host mirror has
the reference's surface (names, shapes, optimiser groups), and the product path refuses to run without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import make_model, load_meta


def _header_prototypes():
    """[(name, return type, kinds)] of every prototype of include/nvfi_hip.h in the header's order: comments and preprocessor lines stripped,
    then `ret name(params);`.  kinds: one letter per parameter - p for anything with a `*`, l int64_t, i int, f float (a scalar of another
    type is a KeyError: the binding's table has no letter for it); `(void)` gives the empty string."""
    txt = open(os.path.join(ROOT, "include", "nvfi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(line for line in txt.split("\n") if not line.lstrip().startswith("#"))
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(nvfi_\w+)\s*\(([^()]*)\)\s*;", txt):
        params = [" ".join(p.split()) for p in params.split(",")]
        kinds = "" if params == ["void"] else "".join(
            "p" if "*" in p else {"int64_t": "l", "int": "i", "float": "f"}[p.rsplit(" ", 1)[0]] for p in params)
        out.append((name, " ".join(ret.split()), kinds))
    return out


def test_library_exports_every_declared_symbol():
    import ctypes as C
    from nvfi_amd import _lib
    from nvfi_amd.build import build
    build()
    L = C.CDLL(_lib.SO)
    names = [n for n, _, _ in _header_prototypes()]
    assert len(names) == len(set(names)) == 75
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/nvfi_hip.h but not exported"
    assert set(_lib.EXPORTS) == set(names) and len(_lib.EXPORTS) == 75
    assert _lib.lib().nvfi_abi_version() == 5 == _lib.ABI_VERSION


def test_signature_table_matches_header():
    """_lib.SIGNATURES is the header: the same 75 names in the same order, every row the header's parameter kinds position by position; and
    lib() has turned every row into argtypes (restype stays ctypes' int except where the header returns something else)."""
    import ctypes as C
    from nvfi_amd import _lib
    protos = _header_prototypes()
    assert list(_lib.SIGNATURES) == [n for n, _, _ in protos] and _lib.EXPORTS == list(_lib.SIGNATURES)
    kind_of = {"p": C.c_void_p, "l": C.c_int64, "i": C.c_int, "f": C.c_float}
    L = _lib.lib()
    for name, ret, kinds in protos:
        assert _lib.SIGNATURES[name] == kinds, (name, _lib.SIGNATURES[name], kinds)
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(kinds), name
        assert list(fn.argtypes) == [kind_of[k] for k in kinds], name
        if name == "nvfi_last_error":
            assert ret == "const char*" and fn.restype is C.c_char_p
        else:
            assert ret == "int" and fn.restype is C.c_int, (name, ret)
    assert isinstance(L.nvfi_last_error(), bytes)


def test_wrong_scalar_kind_is_refused_before_the_call():
    """With argtypes set a wrapper of the wrong kind does not reach the library: ctypes raises while it converts the arguments, so nothing is
    launched (no GPU needed).  One size query of each former group: nvfi_ray_distortion_workspace_bytes had a hand-written argtypes row,
    nvfi_segloss_workspace_bytes had none."""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    nb = C.c_int64(-1)
    for call in (
        lambda: L.nvfi_ray_distortion_workspace_bytes(C.c_int(2048), C.byref(nb)),          # c_int for an int64_t
        lambda: L.nvfi_segloss_workspace_bytes(C.c_int(2048), 4, 8, C.byref(nb)),
        lambda: L.nvfi_segloss_workspace_bytes(2048, 4.0, 8, C.byref(nb)),                  # a Python float for an int
        lambda: L.nvfi_ray_distortion_workspace_bytes(2048.0, C.byref(nb)),                 # ... and for an int64_t
        lambda: L.nvfi_ray_distortion(8, 4, None, C.c_double(0.1), 1.0, None, None, None, None, None, 0, None),     # c_double for a float
        lambda: L.nvfi_knn_self(8, None, 4, C.c_double(0.1), None, None, None, None, None, 0, None),
    ):
        with pytest.raises(C.ArgumentError):
            call()
        assert nb.value == -1
    # plain numbers and correct wrappers both pass
    assert L.nvfi_ray_distortion_workspace_bytes(2048, C.byref(nb)) == 0 and nb.value >= 2048 * 8
    assert L.nvfi_ray_distortion_workspace_bytes(C.c_int64(2048), C.byref(nb)) == 0
    assert L.nvfi_segloss_workspace_bytes(2048, 4, 8, C.byref(nb)) == 0 and nb.value > 0
    assert _lib.bytes_of(L.nvfi_segloss_workspace_bytes, 2048, 4, 8) == nb.value


def test_abi_version_is_checked_at_load(monkeypatch):
    """lib() refuses a library whose nvfi_abi_version() is not the binding's ABI_VERSION, naming both numbers and the file"""
    from nvfi_amd import _lib
    _lib.lib()
    monkeypatch.setattr(_lib, "ABI_VERSION", 6)
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(_lib.NvfiError) as e:
        _lib.lib()
    assert "5" in str(e.value) and "6" in str(e.value) and _lib.SO in str(e.value)
    assert _lib._LIB is None
    monkeypatch.undo()
    assert _lib.ABI_VERSION == 5 and _lib.lib().nvfi_abi_version() == 5


def test_struct_layout_matches_header():
    """every ctypes mirror of a struct of the header has the size the C compiler gives it"""
    import subprocess, tempfile, ctypes as C
    from nvfi_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nvfi_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(nvfi_field_desc), '
           'sizeof(nvfi_grads), sizeof(nvfi_draw_desc), offsetof(nvfi_field_desc, frags), offsetof(nvfi_draw_desc, points), '
           'sizeof(nvfi_mask_desc), sizeof(nvfi_mask_grads), sizeof(nvfi_adam_tensor));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        a, b, c, o1, o2, md, mg, at = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    print("sizeof: mask_desc", md, C.sizeof(_lib.MaskDesc), "mask_grads", mg, C.sizeof(_lib.MaskGrads), "adam_tensor", at, C.sizeof(_lib.AdamTensor))
    assert C.sizeof(_lib.FieldDesc) == a and C.sizeof(_lib.Grads) == b and C.sizeof(_lib.DrawDesc) == c
    assert _lib.FieldDesc.frags.offset == o1 and _lib.DrawDesc.points.offset == o2      # ABI v5 additions
    assert C.sizeof(_lib.MaskDesc) == md and C.sizeof(_lib.MaskGrads) == mg and C.sizeof(_lib.AdamTensor) == at


@pytest.mark.parametrize("kind", ["A", "B"])
def test_state_dict_surface(kind):
    model, meta = make_model(kind, device="cpu")
    _, sd = load_meta(kind)
    own = model.state_dict()
    for k, v in sd.items():
        assert k in own and tuple(own[k].shape) == tuple(v.shape), k
    # the reference registers vel_net twice (tensorf_keyframe.py:94,106): duplicated keys must exist
    assert "nvfi.vel.vel_net.weight_net.1.weight" in own and "nvfi.vel_net.weight_net.1.weight" in own
    f = model.nvfi
    for p in list(f.density_plane_space) + list(f.app_plane_time):
        assert p.is_contiguous(memory_format=torch.channels_last)     # physical [H][W][C]
    groups = model.get_optparam_groups(0.02, 1e-3)
    assert [g["lr"] for g in groups] == [0.02] * 4 + [1e-3] * 4
    assert type(f.vel).__name__ == ("VelocityAABBSur" if kind == "B" else "VelocityAABB")
    kw = f.get_kwargs()
    assert kw["gridSize"] == [int(g) for g in meta["gridSize"]] and kw["num_keyframes"] == int(meta["num_keyframes"])


def test_no_cpu_fallback():
    from nvfi_amd._lib import NvfiError
    model, _ = make_model("A", device="cpu")
    with pytest.raises(NvfiError):
        model.render_ray(0.3, torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(NvfiError):
        model.get_vel_loss(64)


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under nvfi_amd/ may reference it"""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "nvfi_amd")):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h")):
                if re.search(r"\boracle\b", open(os.path.join(dp, fn), errors="ignore").read()):
                    bad.append(fn)
    assert not bad, bad


def test_upsample_keeps_layout_and_matches_reference_formula():
    model, _ = make_model("A", device="cpu")
    f = model.nvfi
    before = f.density_plane_space[0].detach().clone()
    f.upsample_volume_grid([26, 24, 22], 4)
    p = f.density_plane_space[0]
    assert tuple(p.shape) == (1, 24, 24, 26) and p.is_contiguous(memory_format=torch.channels_last)
    ref = torch.nn.functional.interpolate(before, size=(24, 26), mode="bilinear", align_corners=True)
    assert torch.allclose(p, ref)
    assert f.gridSize.tolist() == [26, 24, 22] and f._step_host == float(f.stepSize)


def test_checkpoint_round_trip(tmp_path):
    """f-4: the reference's checkpoint dictionary layout; planes come back channels_last with identical values"""
    from nvfi_amd.utils import save_checkpoint, load_checkpoint, load_model_checkpoint
    from helpers import field_cfg
    model, meta = make_model("A", device="cpu")
    opt = torch.optim.Adam(model.get_optparam_groups(), betas=(0.9, 0.99))
    path = save_checkpoint(str(tmp_path), model, opt, epoch=12)
    assert path.endswith("model_00012.ckpt")
    ck = load_checkpoint(str(tmp_path))
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "nvfi_kwarg"}
    assert ck["model_state_dict"]["nvfi.density_plane_space.0"].is_contiguous()    # logical NCHW on disk
    m2, _ = load_model_checkpoint(field_cfg(meta), ck, "cpu")
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert m2.nvfi.density_plane_space[0].is_contiguous(memory_format=torch.channels_last)
    # with an occupancy mask: the loader rebuilds AlphaGridMask from the state_dict keys and loads STRICTLY (train_nvfi.py:380-386)
    from nvfi_amd.models import AlphaGridMask
    gs = [int(g) for g in meta["gridSize"]]
    vol = (torch.rand(gs[2], gs[1], gs[0]) > 0.4).float()
    model.nvfi.alphaMask = AlphaGridMask("cpu", model.nvfi.aabb, vol)
    save_checkpoint(str(tmp_path), model, opt, epoch=13)
    ck = load_checkpoint(str(tmp_path))
    assert "nvfi.alphaMask.alpha_volume" in ck["model_state_dict"] and "alphaMask_grid" in ck["nvfi_kwarg"]
    m3, _ = load_model_checkpoint(field_cfg(meta), ck, "cpu")
    assert m3.nvfi.alphaMask is not None and torch.equal(m3.nvfi.alphaMask.alpha_volume.reshape(vol.shape), vol)
    assert m3.nvfi.nSamples == model.nvfi.nSamples and m3.nvfi._aabb_host == model.nvfi._aabb_host
    bad = dict(ck); bad["model_state_dict"] = dict(ck["model_state_dict"]); bad["model_state_dict"]["nvfi.bogus"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        load_model_checkpoint(field_cfg(meta), bad, "cpu")


def test_camera_rays_match_reference(gold):
    """f-2: Camera.get_ray_bundle against the reference's rays (models/camera.py:112-138) - the strided centre crop of the 800x800
    camera that tests/golden/make_golden.py stored as `A:rays_o/d`, `B:rays_o/d` (and `nvfi_gen_rays` is tested against this
    Camera on the GPU, so the device-side generator inherits the pin)."""
    import bench
    from nvfi_amd.models import Camera
    full, stride, H = 800, 24, 16
    focal = 0.5 * full / np.tan(0.5 * 0.6911112)
    for kind, center in (("A", (0.0, 0.0, 0.0)), ("B", (0.0, 0.0, 3.0))):
        pose = bench.pose_spherical(30.0, -30.0, 4.0)
        pose[:3, 3] += torch.tensor(center)
        cam = Camera(pose, full, full, focal, torch.zeros(1, 1, 3), 1.0, 8.0)
        i0 = full // 2 - (H // 2) * stride
        sl = slice(i0, i0 + H * stride, stride)
        o = cam.rays.ray_origins[sl, sl].reshape(-1, 3).numpy()
        d = cam.rays.ray_directions[sl, sl].reshape(-1, 3).numpy()
        assert np.array_equal(o, gold[f"{kind}:rays_o"]) and np.array_equal(d, gold[f"{kind}:rays_d"]), kind


def test_boundary_ray_types():
    """`from models import *` of the reference exposes Ray, Camera, BatchedRays (models/__init__.py:1): containers behave alike"""
    import torch
    from nvfi_amd.models import BatchedRays, Camera, Ray
    pose = torch.eye(4)
    img = torch.rand(4, 5, 3)
    b = BatchedRays([img, img * 0.5], [pose, pose], [0.1, 0.2], 4, 5, 3.0, 1.0, 8.0)
    assert len(b) == 40 and b.all_rays.shape == (40, 6) and b.all_pixels.shape == (40, 3) and b.all_ts.shape == (40, 1)
    assert float(b.all_ts[0]) == pytest.approx(0.1) and float(b.all_ts[-1]) == pytest.approx(0.2)
    cam = Camera(pose, 4, 5, 3.0, img, 1.0, 8.0)
    assert torch.equal(b.all_rays[:20, 3:], cam.rays.ray_directions.reshape(-1, 3))
    r = Ray(torch.zeros(7, 3), torch.ones(7, 3), 1.0, 8.0)
    p = r.points_sampling(6, perturb=False)
    assert p.shape == (7, 6, 3) and float(p[0, 0, 0]) == pytest.approx(1.0) and float(p[0, -1, 0]) == pytest.approx(8.0)
    r.update_near_far(torch.full((7, 1), 2.0), torch.full((7, 1), 4.0))     # buffers: tensors, as in the reference
    assert float(r.near[0]) == 2.0 and float(r.far[0]) == 4.0


def test_bench_spawn_helper_refuses_more_ranks_than_gpus(capsys):
    """bench.py --gpus N starts N RCCL ranks itself; with fewer devices than ranks it must say so and fail (not run one process)."""
    import bench
    assert bench._spawn_ranks(8, 1, "nccl") == 2
    assert "needs 8 GPUs" in capsys.readouterr().err


def test_rccl_comm_needs_a_process_group_for_the_bootstrap():
    from nvfi_amd import _lib
    from nvfi_amd.dist import RcclComm
    with pytest.raises(_lib.NvfiError, match="init_process_group"):
        RcclComm(world=2, rank=1)


def test_traffic_classes_match_the_committed_counter_pass(tmp_path):
    """bench.py quotes roofline.traffic from profiles/<tag>_traffic.json, which tools/make_traffic.py derives from the committed FETCH_SIZE /
    WRITE_SIZE summaries by kernel name.  A renamed kernel (new template arguments) must not silently turn a class into 0 bytes: every
    class the current default path launches has to match a kernel of the committed trace, and the dominant class has to carry bytes."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_traffic", os.path.join(ROOT, "tools", "make_traffic.py"))
    mt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mt)
    bench_src = open(os.path.join(ROOT, "bench.py")).read()
    tag = re.search(r'^PROFILE_TAG = "(\w+)"', bench_src, re.M).group(1)
    prof = os.path.join(ROOT, "profiles")
    out = tmp_path / "traffic.json"
    mt.main(os.path.join(prof, f"{tag}_pmc_fetch_size.csv"), os.path.join(prof, f"{tag}_pmc_write_size.csv"), str(out), "test")
    fresh = json.load(open(out))["bytes_per_launch"]
    assert all(v is not None and v > 0 for v in fresh.values()), fresh
    committed = json.load(open(os.path.join(prof, f"{tag}_traffic.json")))["bytes_per_launch"]
    assert committed == pytest.approx(fresh)
    assert committed["pde_prefilter"] > 1e6


def test_train_short_circuit_sees_mode_changes_made_on_the_inner_field():
    """NVFi.train() returns early for an unchanged mode (train_nvfi.py:141-142 calls it every iteration), but a mode set on the inner field -
    model.nvfi.eval(), as tests and the golden scripts do - or on a module attached later must not survive the next model.train()"""
    m, _ = make_model("A", "cpu")
    m.train()
    assert m.nvfi.training and m.nvfi.vel_net.training
    m.train()                                   # the short-circuit path
    m.nvfi.eval()                               # behind the wrapper's back
    assert not m.nvfi.training and m.training
    m.train()
    assert m.nvfi.training and all(c.training for c in m.nvfi.modules())
    m.eval(); m.eval()
    m.nvfi.renderModule.train()                 # one direct child flipped
    m.eval()
    assert not any(c.training for c in m.modules())
    m.train()
    from nvfi_amd.models.mask_field import MaskField
    m.nvfi.mask_field = MaskField(4).eval()     # attached later, in another mode
    m.train()
    assert m.nvfi.mask_field.training


def test_gradient_arena_is_opt_in():
    """the default autograd contract of a drop-in nn.Module: gradients go back to the engine (torch.autograd.grad, hooks); the in-place
    arena is something a driver switches on (NVFI_INPLACE_GRADS=arena, bench.py --mode dropin, tools/run_reference_driver.py)"""
    m, _ = make_model("A", "cpu")
    assert m.nvfi.accumulate_grads_inplace is False
    src = open(os.path.join(ROOT, "tools", "run_reference_driver.py")).read()
    assert 'setdefault("NVFI_INPLACE_GRADS", "arena")' in src and "--pure-autograd" in src


def test_ray_lazy_buffers_follow_the_module_and_camera_attributes_are_assignable():
    from nvfi_amd.models import Ray, Camera
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    r = Ray(o, d, torch.full((5, 1), 2.0), 6.0, t=torch.full((5, 1), 0.25))
    r2 = r.to(torch.float64)                                   # pending tensors are converted with the buffers
    assert r2.near.dtype == torch.float64 and r2.t.dtype == torch.float64 and r2.far.dtype == torch.float64
    assert set(Ray(o, d, 2.0, 6.0).state_dict()) == {"ray_origins", "ray_directions", "near", "far", "t"}
    cam = Camera(torch.eye(4), 4, 6, 5.0, torch.zeros(4, 6, 3), 2.0, 6.0)
    rays = cam.rays
    cam.rays = rays; cam.coords = cam.coords                   # attributes in the reference, assignable here too
    assert cam.rays is rays


def test_switch_table_matches_the_integration_guide_and_is_the_only_reader():
    """csrc/switches.h is the one table of the environment variables the library reads: INTEGRATION section 4 shows the same default for every
    row, abi.hip's reader is the only getenv of csrc/, the per-device set-up of a launcher goes through common.h's DeviceOnce, and no launcher keeps a retired sweep switch alive as a
    `static int x = -1` selector or a kernel alive by explicit instantiation (text only)."""
    csrc = os.path.join(ROOT, "nvfi_amd", "csrc")
    rows = re.findall(r"^\s*X\((NVFI_\w+),\s*(INT|WORD),\s*(\w+)\)", open(os.path.join(csrc, "switches.h")).read(), flags=re.M)
    assert len(rows) == 16 and len({name for name, _, _ in rows}) == 16, rows
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = guide[guide.index("## 4. Environment switches of the library"):]
    documented = {}
    for line in section.splitlines():
        cells = [c.strip() for c in line.split("|")]
        if len(cells) < 4 or not cells[1].startswith("`NVFI_"):
            continue
        names, defaults = re.findall(r"`(NVFI_\w+)`", cells[1]), re.findall(r"`([^`]*)`", cells[2])
        if len(names) == len(defaults):             # (a row may list two variables: `A`, `B` | `1`, `1`)
            documented.update(zip(names, defaults))
    for name, _, default in rows:
        assert documented.get(name) == default, f"{name}: switches.h says {default}, INTEGRATION section 4 says {documented.get(name)}"
    sources = {fn: open(os.path.join(csrc, fn), errors="ignore").read() for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h"))}
    assert [fn for fn, txt in sources.items() if "getenv" in txt] == ["abi.hip"]
    assert sources["abi.hip"].count("getenv") == 1
    old_idiom = {fn: [w for w in ("static bool done", "static bool attr", "hipFuncSetAttribute") if w in txt and (fn, w) != ("common.h", "hipFuncSetAttribute")]
                 for fn, txt in sources.items()}
    old_idiom = {fn: w for fn, w in old_idiom.items() if w}
    assert not old_idiom, old_idiom
    # retired sweep switches leave nothing behind: no `static int x = -1;` selector in a launcher (the variant it chose would still be
    # compiled), and no explicit instantiation that keeps a kernel without a launcher in the library
    selectors = {fn: re.findall(r"static\s+int\s+\w+\s*=\s*-\s*1\s*;", txt) for fn, txt in sources.items()}
    selectors = {fn: w for fn, w in selectors.items() if w}
    assert not selectors, selectors
    kept = {fn: re.findall(r"^\s*template\s+(?!<)[^;{]*\bk_\w+[^;{]*;", txt, flags=re.M) for fn, txt in sources.items()}
    kept = {fn: w for fn, w in kept.items() if w}
    assert not kept, kept


def test_reduction_and_point_wave_idioms_have_one_home():
    """The device idioms of the loss and metric units are defined once (text only): the fp64 wave butterfly in reduce.h (common.h keeps its
    float one), the ticket arrival that drains with s_waitcnt vmcnt(0) in reduce.h, and prod6 / the odd LDS stride of basis_mat / the
    other-five product of the wave-per-point family in pointwave.h (scatter_atomic.hip, the render backward's scatter, keeps its own)."""
    csrc = os.path.join(ROOT, "nvfi_amd", "csrc")
    code = {fn: re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, fn), errors="ignore").read(), flags=re.S)
            for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h"))}
    assert "reduce.h" in code and "pointwave.h" in code
    kinds = r"\b(?:double|float|int|unsigned|T)\b"

    def summed_types(txt):      # type of every X in `for (int o = 32; o > 0; o >>= 1) X += __shfl_xor(X, o)`: its nearest declaration in front
        out = []
        for m in re.finditer(r"for\s*\(\s*int\s+o\s*=\s*32\s*;\s*o\s*>\s*0\s*;\s*o\s*>>=\s*1\s*\)\s*\{?\s*(\w+)(\[\w+\])?\s*\+=\s*__shfl_xor\(\s*\1", txt):
            decl = re.findall(r"(%s)(?:(?!%s)[^;(){}])*?\b%s\b" % (kinds, kinds, m.group(1)), txt[:m.start()])
            out.append(decl[-1] if decl else "?")
        return out

    types = {fn: summed_types(txt) for fn, txt in code.items()}
    assert types["reduce.h"] == ["T"] and types["common.h"] == ["float"], (types["reduce.h"], types["common.h"])
    elsewhere = {fn: t for fn, t in types.items() if fn not in ("common.h", "reduce.h") and any(k in ("double", "T", "?") for k in t)}
    assert not elsewhere, f"a wave butterfly over a double outside reduce.h: {elsewhere}"
    # a function that returns "I am the last workgroup" after draining its stores: reduce.h's last_arrival only; the loss and metric units
    # have no drain and no ticket draw of their own
    arrivals = {fn: re.findall(r"\bbool\s+(\w+)\s*\(\s*int\s*\*\s*ticket[^)]*\)\s*\{[^}]*s_waitcnt vmcnt\(0\)", txt) for fn, txt in code.items()}
    assert {fn: a for fn, a in arrivals.items() if a} == {"reduce.h": ["last_arrival"]}, arrivals
    for fn in ("segloss.hip", "metrics.hip", "charloss.hip", "depthloss.hip", "raydist.hip", "flowloss.hip", "lookup.hip"):
        assert "s_waitcnt" not in code[fn] and "__hip_atomic_fetch_add" not in code[fn], fn
    homes = {"pointwave.h", "scatter_atomic.hip"}
    for what, pattern in (("prod6", r"\bfloat\s+prod6\s*\("), ("stride 49", r"\b49\b"), ("other-five product", r"L\[p\]\s*=\s*L\[p - 1\]\s*\*\s*val\[p - 1\]")):
        found = {fn for fn, txt in code.items() if re.search(pattern, txt)}
        assert "pointwave.h" in found and found <= homes, f"{what}: {sorted(found)}"


def test_warp_dispatch_has_one_home():
    """The host side of the velocity warp is warp.hip's (text only, comments stripped): the argument blocks of the single warp kernels are named
    in their defining units, in warp.hip and - X6Args, the PDE prefilter - in pde.hip; the fp32 and fp16-input launchers are called from
    warp.hip and, once each, from nvfi_compute_alpha's fixed-schedule branch in abi.hip; warp.hip defines no kernel; the point limit of a call
    is spelled out once; nvfi_render_flow counts RK2 steps with common.h's rk_steps, not with a loop of its own."""
    csrc = os.path.join(ROOT, "nvfi_amd", "csrc")
    code = {fn: re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, fn), errors="ignore").read(), flags=re.S)
            for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h"))}
    assert "warp.hip" in code and "warp.h" in code
    blocks = {"X6Args": {"x6.h", "vel_x6.hip", "vel_x6w.hip", "warp.hip", "pde.hip"}, "X6UniArgs": {"x6.h", "vel_x6.hip", "vel_x6w.hip", "warp.hip"},
              "SplitUniArgs": {"pde.h", "vel_split.hip", "warp.hip"}, "SplitBwdArgs": {"pde.h", "vel_split.hip", "warp.hip"}}
    for name, homes in blocks.items():
        found = {fn for fn, txt in code.items() if re.search(r"\b%s\b" % name, txt)}
        assert "warp.hip" in found and found <= homes, f"{name}: {sorted(found - homes)}"
    for call, own in (("launch_rk2_fwd(", {"vel.h", "vel.hip"}), ("launch_rk2_inf16(", {"pde.h", "pre16.hip"})):
        counts = {fn: txt.count(call) for fn, txt in code.items() if call in txt and fn not in own}
        assert set(counts) == {"warp.hip", "abi.hip"} and counts["abi.hip"] == 1, f"{call}: {counts}"
    assert "__global__" not in code["warp.hip"] and "__global__" not in code["warp.h"]
    spelled = {fn: txt.count("(1ll << 31) - 256") for fn, txt in code.items() if "(1ll << 31) - 256" in txt}
    assert spelled == {"common.h": 1}, spelled
    assert not re.search(r"\bwhile\b", code["flow.hip"])


def _plan_desc():
    """nvfi_field_desc with the sizes of golden field A and no pointers: the workspace plan reads sizes only"""
    from nvfi_amd import _lib
    f = make_model("A", device="cpu")[0].nvfi
    d = _lib.FieldDesc()
    d.G[:] = f._grid_host
    d.K, d.Cd, d.Ca, d.app_dim = int(f.num_keyframes), int(f.density_n_comp[0]), int(f.app_n_comp[0]), int(f.app_dim)
    d.n_samples, d.use_vel, d.tmax = int(f.nSamples), 1, float(f.tmax)
    return d


def _plan_bytes(d, R, flags, t=None):
    """(return code, bytes) of nvfi_render_workspace_bytes (t None) / nvfi_render_workspace_bytes_t"""
    import ctypes as C
    from nvfi_amd import _lib
    nb = C.c_int64(-1)
    if t is None:
        rc = _lib.lib().nvfi_render_workspace_bytes(C.byref(d), C.c_int64(R), C.c_int(flags), C.byref(nb))
    else:
        rc = _lib.lib().nvfi_render_workspace_bytes_t(C.byref(d), C.c_int64(R), C.c_int(flags), C.c_float(t), C.byref(nb))
    return rc, nb.value


def _plan_cases(d):
    """name -> (R, flags, t): R in {5, 8192, 8193}, seven flag sets, the t-independent bound and three times - a keyframe time, one half an RK2
    step off a keyframe, one two steps past the last keyframe (dt_max = half a keyframe interval)"""
    from nvfi_amd import _lib as L
    ts = np.float32(d.tmax) / np.float32(d.K - 1)
    dtm = np.float32(0.5) * ts
    times = {"any": None, "key": float(ts), "half": float(ts + np.float32(0.5) * dtm), "two": float(np.float32(d.tmax) + np.float32(2) * dtm)}
    flagsets = {"0": 0, "T": L.NVFI_TRAIN, "TF": L.NVFI_TRAIN | L.NVFI_BWD_FORK, "M": L.NVFI_WANT_MASK, "F": L.NVFI_WANT_FLOW, "S": L.NVFI_WANT_SELECT,
                "MFS": L.NVFI_WANT_MASK | L.NVFI_WANT_FLOW | L.NVFI_WANT_SELECT}
    return {f"{R}:{fn}:{tn}": (R, fl, t) for R in (5, 8192, 8193) for fn, fl in flagsets.items() for tn, t in times.items()}


# bytes of the plan before render.hip was split into units (the library of the commit before, same calls, default switches)
PLAN_BYTES = {
    "5:0:any": 885248, "5:0:key": 885248, "5:0:half": 1600256, "5:0:two": 1600256,
    "5:T:any": 215480320, "5:T:key": 104312576, "5:T:half": 211329024, "5:T:two": 215480320,
    "5:TF:any": 215480320, "5:TF:key": 104312576, "5:TF:half": 211329024, "5:TF:two": 215480320,
    "5:M:any": 1185280, "5:M:key": 1185280, "5:M:half": 1900288, "5:M:two": 1900288,
    "5:F:any": 1320192, "5:F:key": 1320192, "5:F:half": 2035200, "5:F:two": 2035200,
    "5:S:any": 1148672, "5:S:key": 1148672, "5:S:half": 1863680, "5:S:two": 1863680,
    "5:MFS:any": 1883648, "5:MFS:key": 1883648, "5:MFS:half": 2598656, "5:MFS:two": 2598656,
    "8192:0:any": 23405568, "8192:0:key": 23405568, "8192:0:half": 26600704, "8192:0:two": 26600704,
    "8192:T:any": 13467959552, "8192:T:key": 2895663104, "8192:T:half": 8234483968, "8192:T:two": 13467959552,
    "8192:TF:any": 13467959552, "8192:TF:key": 2895663104, "8192:TF:half": 8234483968, "8192:TF:two": 13467959552,
    "8192:M:any": 85533696, "8192:M:key": 85533696, "8192:M:half": 88728832, "8192:M:two": 88728832,
    "8192:F:any": 50889728, "8192:F:key": 50889728, "8192:F:half": 54084864, "8192:F:two": 54084864,
    "8192:S:any": 25601024, "8192:S:key": 25601024, "8192:S:half": 28796160, "8192:S:two": 28796160,
    "8192:MFS:any": 115213312, "8192:MFS:key": 115213312, "8192:MFS:half": 118408448, "8192:MFS:two": 118408448,
    "8193:0:any": 23410176, "8193:0:key": 23410176, "8193:0:half": 26606080, "8193:0:two": 26606080,
    "8193:T:any": 13471280128, "8193:T:key": 2896221184, "8193:T:half": 8236423680, "8193:T:two": 13471280128,
    "8193:TF:any": 13471280128, "8193:TF:key": 2896221184, "8193:TF:half": 8236423680, "8193:TF:two": 13471280128,
    "8193:M:any": 85545984, "8193:M:key": 85545984, "8193:M:half": 88741888, "8193:M:two": 88741888,
    "8193:F:any": 50897920, "8193:F:key": 50897920, "8193:F:half": 54093824, "8193:F:two": 54093824,
    "8193:S:any": 25605888, "8193:S:key": 25605888, "8193:S:half": 28801792, "8193:S:two": 28801792,
    "8193:MFS:any": 115229440, "8193:MFS:key": 115229440, "8193:MFS:half": 118425344, "8193:MFS:two": 118425344,
}


def test_render_workspace_layout_is_pinned():
    """The workspace plan of a render call (plan_render behind render_plan_at, render.hip) is shared by the forward, the backward and the
    branches that read the forward's workspace, and by callers that size it: its byte counts for golden field A's sizes are literals.  A time
    that needs more than MAX_RK_STEPS (64) RK2 steps is refused with code 2."""
    d = _plan_desc()
    cases = _plan_cases(d)
    assert len(cases) == 3 * 7 * 4 and set(cases) == set(PLAN_BYTES)
    got = {k: _plan_bytes(d, *c) for k, c in cases.items()}
    assert all(rc == 0 for rc, _ in got.values()), {k: v for k, v in got.items() if v[0]}
    assert {k: v[1] for k, v in got.items()} == PLAN_BYTES
    dtm = 0.5 * d.tmax / (d.K - 1)
    rc, _ = _plan_bytes(d, 8, 0, d.tmax + 65.5 * dtm)
    from nvfi_amd import _lib
    assert rc == 2 and b"RK2 steps" in _lib.lib().nvfi_last_error()
    assert _plan_bytes(d, 8, 0, d.tmax + 63.5 * dtm)[0] == 0


# bytes of the point calls' workspaces and of the fragment cache in the library of the commit before vel_images() (frags.h) became the one
# way to the velocity net's weight images, for N / P = 1, 255, 256, 4096, 262144, 262145
POINT_SIZES = (1, 255, 256, 4096, 262144, 262145)
POINT_BYTES = {
    "nvfi_pde_workspace_bytes": (311206912, 315375360, 315375360, 440198656, 8828347392, 8828351488),
    "nvfi_vel_workspace_bytes": (1161472, 1168384, 1168384, 1275904, 8501248, 8501504),
    "nvfi_alpha_workspace_bytes": (997120, 1003520, 1003520, 1111040, 8336384, 8337152),
    "nvfi_char_workspace_bytes": (1162496, 1173760, 1173760, 1358080, 13744384, 13745408),
}
FRAG_CACHE_BYTES = 3125504
X4_T0_BYTES = 1 * (64 // 4) * 256 * 4      # the x4 copy of weight_net's transposed input layer: 1 tile x 64 K steps (pde.h: X4_FLOATS(1, 64))
# bytes of the adjoint chains' workspaces for N / R = 1, 128, 129, 4096, generated by running these queries on the library of the commit before
# warp.h took over the image rooms of plan_advect / plan_flow_loss (default switches).  "<query>:<own|cached>:<RK2 steps>": own - frags NULL, the
# call packs the images into its own rooms; cached - a non-NULL frags (the size queries test the pointer only)
CHAIN_SIZES = (1, 128, 129, 4096)
CHAIN_BYTES = {
    "nvfi_advect_grad_workspace_bytes:own:1": (104106240, 104119808, 105496832, 147228160),
    "nvfi_advect_grad_workspace_bytes:own:2": (105482496, 105505792, 108259072, 191579648),
    "nvfi_advect_grad_workspace_bytes:cached:1": (102827264, 102840832, 104217856, 145949184),
    "nvfi_advect_grad_workspace_bytes:cached:2": (104203520, 104226816, 106980096, 190300672),
    "nvfi_advect_grad_pt_workspace_bytes:own:1": (104106496, 104120832, 105498112, 147260928),
    "nvfi_advect_grad_pt_workspace_bytes:own:2": (105482752, 105507840, 108261376, 191645184),
    "nvfi_advect_grad_pt_workspace_bytes:cached:1": (102827520, 102841856, 104219136, 145981952),
    "nvfi_advect_grad_pt_workspace_bytes:cached:2": (104203776, 104228864, 106982400, 190366208),
    "nvfi_flow_loss_workspace_bytes:own:1": (104528640, 104963328, 106344704, 161261312),
    "nvfi_flow_loss_workspace_bytes:own:2": (105904896, 106349312, 109106944, 205612800),
    "nvfi_flow_loss_workspace_bytes:cached:1": (102831872, 103266560, 104647936, 159564544),
    "nvfi_flow_loss_workspace_bytes:cached:2": (104208128, 104652544, 107410176, 203916032),
}


def _chain_bytes(d):
    """the three size queries of the adjoint chains for _plan_desc(): nvfi_advect_grad (t one half / one and a half RK2 steps from t_target),
    nvfi_advect_grad_pt (max_steps 1 / 2), nvfi_flow_loss (dt likewise, chunk_cap = R)"""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    dtm = np.float32(0.5) * np.float32(d.tmax) / np.float32(d.K - 1)
    got = {}
    for room, frags in (("own", None), ("cached", 256)):
        d.frags = frags
        for steps in (1, 2):
            span = C.c_float(float((np.float32(steps) - np.float32(0.5)) * dtm))
            queries = {
                "nvfi_advect_grad_workspace_bytes": lambda n, nb: L.nvfi_advect_grad_workspace_bytes(C.byref(d), C.c_int64(n), span, C.c_float(0.0), nb),
                "nvfi_advect_grad_pt_workspace_bytes": lambda n, nb: L.nvfi_advect_grad_pt_workspace_bytes(C.byref(d), C.c_int64(n), C.c_int(steps), nb),
                "nvfi_flow_loss_workspace_bytes": lambda n, nb: L.nvfi_flow_loss_workspace_bytes(C.byref(d), C.c_int64(n), C.c_float(0.0), span, C.c_int64(n), nb),
            }
            for name, query in queries.items():
                row = []
                for n in CHAIN_SIZES:
                    nb = C.c_int64(-1)
                    assert query(n, C.byref(nb)) == 0, (name, room, steps, n, L.nvfi_last_error())
                    row.append(nb.value)
                got[f"{name}:{room}:{steps}"] = tuple(row)
    d.frags = None
    return got


def test_point_workspace_sizes_are_pinned():
    """The published workspace sizes of the PDE term, nvfi_vel_eval / nvfi_integrate_pos, nvfi_compute_alpha and the characteristic loss, and the
    size of the fragment cache, for golden field A's sizes are literals of the parent library.  One moved on purpose: an uncached PDE call packs
    weight_net's whole transposed x4 set - T0 travels with it, although no PDE kernel reads it - so its workspace is 16 KB larger at every P.
    The adjoint chains (nvfi_advect_grad, nvfi_advect_grad_pt, nvfi_flow_loss_*), whose image rooms come from warp.h's need table: CHAIN_BYTES,
    with and without a fragment cache, for one and two RK2 steps."""
    import ctypes as C
    from nvfi_amd import _lib
    d = _plan_desc()
    assert _chain_bytes(d) == CHAIN_BYTES
    assert X4_T0_BYTES == 16384
    for name, want in POINT_BYTES.items():
        got = []
        for n in POINT_SIZES:
            nb = C.c_int64(-1)
            assert getattr(_lib.lib(), name)(C.byref(d), C.c_int64(n), C.byref(nb)) == 0, name
            got.append(nb.value)
        grow = X4_T0_BYTES if name == "nvfi_pde_workspace_bytes" else 0
        assert tuple(got) == tuple(w + grow for w in want), name
    nb = C.c_int64(-1)
    assert _lib.lib().nvfi_frag_cache_bytes(C.byref(d), C.byref(nb)) == 0 and nb.value == FRAG_CACHE_BYTES


def test_point_queries_refuse_before_anything_is_launched():
    """nvfi_vel_eval / nvfi_integrate_pos on a field without a velocity net (its vW / vb / aW / ab are NULL), on a descriptor check_desc rejects and
    on N >= 2^31 - 256; the N limit at nvfi_density_at / nvfi_app_at / nvfi_render_mlp: error 2 with a message, returned before the first HIP
    call - so this runs where there is no GPU, on host-built descriptors and dummy pointers that nothing may dereference."""
    import ctypes as C
    from nvfi_amd import _lib
    L = _lib.lib()
    L.nvfi_last_error.restype = C.c_char_p
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)
    big = (1 << 31) - 256

    def vel_eval(d, n, gated=0):
        return L.nvfi_vel_eval(C.byref(d), C.c_int64(n), p, p, C.c_int(gated), p, C.c_int64(256), None)

    def integrate(d, n):
        return L.nvfi_integrate_pos(C.byref(d), C.c_int64(n), p, p, p, p, p, C.c_int64(256), None)

    def density(d, n):
        return L.nvfi_density_at(C.byref(d), C.c_int64(n), p, p, p, None)

    def app_at(d, n):
        return L.nvfi_app_at(C.byref(d), C.c_int64(n), p, p, p, p, C.c_int64(256), None)

    def render_mlp(d, n):
        return L.nvfi_render_mlp(C.byref(d), C.c_int64(n), p, p, p, p, p, C.c_int64(256), None)

    def refused(rc, *words):
        msg = L.nvfi_last_error().decode()
        assert rc == 2 and all(w in msg for w in words), (rc, msg)

    # ---- a field without a velocity net: every pointer of the two nets is NULL
    d = _plan_desc()
    d.use_vel = 0
    for gated in (0, 1):
        refused(vel_eval(d, 16, gated), "nvfi_vel_eval", "use_vel")
    refused(integrate(d, 16), "nvfi_integrate_pos", "use_vel")
    refused(integrate(d, 0), "nvfi_integrate_pos", "use_vel")         # the descriptor is checked before the empty call returns 0
    # ---- a descriptor the kernels are not built for
    d = _plan_desc()
    d.Cd = 16
    refused(vel_eval(d, 16), "Cd=16")
    refused(integrate(d, 16), "Cd=16")
    d = _plan_desc()
    d.n_samples = 0
    refused(vel_eval(d, 16), "n_samples")
    refused(integrate(d, 16), "n_samples")
    # ---- N that does not fit the kernels' int counters: the limit of nvfi_compute_alpha, at its first refused value and above
    d = _plan_desc()
    for n in (big, 1 << 31, 1 << 40):
        refused(integrate(d, n), "nvfi_integrate_pos", "N too large")
        refused(density(d, n), "nvfi_density_at", "N too large")
        refused(app_at(d, n), "nvfi_app_at", "N too large")
        refused(render_mlp(d, n), "nvfi_render_mlp", "N too large")
    # ---- one under the limit is NOT refused for its size: the 256-byte workspace is (4), still before any launch
    assert integrate(d, big - 1) == 4 and app_at(d, big - 1) == 4 and render_mlp(d, big - 1) == 4 and vel_eval(d, 1 << 40) == 4
    assert "workspace too small" in L.nvfi_last_error().decode()
    # ---- an empty call stays a no-op
    assert vel_eval(d, 0) == 0 and integrate(d, 0) == 0 and density(d, 0) == 0 and app_at(d, 0) == 0 and render_mlp(d, 0) == 0
