"""CPU checks of the segmentation objective (no GPU): the library exports the new entry points, nvfi_amd.utils.seg_loss has the reference's
surface and refuses CPU tensors, and the float64 yardstick (tests/segloss64.py) is pinned to the reference's own fp32 outputs in
tests/golden/segloss.npz (tests/golden/make_golden_segloss.py; the neighbour tables there come from that script's brute-force shim of
pytorch3d.ops).

Bounds of the pin = 4 x the worst distance of the fp32 reference from the float64 yardstick over the four cases, as the golden script printed it
when the fixture was made:
    dynamic 7.75e-07, smooth 1.27e-07, entropy 7.89e-08 (relative); pc_transformed 4.80e-07, g_dynamic 1.06e-04, g_smooth 1.66e-07,
    g_entropy 1.27e-07 (max of max-norm and L2 relative error); R 6.05e-07, t 1.60e-07 (max abs, objects above the singular-value floor).
g_dynamic is the direction (q - pc2) / |q - pc2| of a residual of about 1e-3 between vectors of size 0.6: the fp32 reference itself loses three
digits there.  Neighbour tables: the yardstick's search equals the shim's on every stored row of every case (0 rows differ; the smallest
relative gap between the k-th and (k+1)-th squared distance is 1.04e-05 on lattice_k16, no distance is within 2.7e-04 of the radius)."""
import inspect
import os

import numpy as np
import pytest
import torch

import segloss64 as s64
from conftest import GOLD, ROOT, maxrel, rel_l2

CASES = ["lattice_k4", "lattice_k16", "small", "zerocol"]
BOUND = {"dynamic": 3.1e-6, "smooth": 5.1e-7, "entropy": 3.2e-7, "pc_transformed": 1.92e-6, "g_dynamic": 4.3e-4, "g_smooth": 6.7e-7,
         "g_entropy": 5.1e-7, "R": 2.5e-6, "t": 6.4e-7}


@pytest.fixture(scope="module")
def sgold():
    return np.load(os.path.join(GOLD, "segloss.npz"))


def load_case(z, name):
    """inputs and stored outputs of one fixture case (lattice_k16 shares lattice_k4's inputs and dynamic / entropy outputs)"""
    src = "lattice_k4" if name == "lattice_k16" else name
    k, radius, norm = z[f"{name}:cfg"]
    c = dict(pc=z[f"{src}:pc"], flow=z[f"{src}:flow"], mask=z[f"{src}:mask"], k=int(k), radius=float(radius), loss_norm=int(norm),
             rows=z[f"{name}:rows"].astype(np.int64), sv_ok=z[f"{name}:sv_ok"], losses=z[f"{name}:losses"], idx=z[f"{name}:idx"].astype(np.int64),
             g_smooth=z[f"{name}:g_smooth"])
    for q in ("pc_transformed", "g_dynamic", "g_entropy", "R", "t"):
        c[q] = z[f"{src}:{q}"]
    c["idx_rows"] = np.arange(c["pc"].shape[0]) if c["idx"].shape[0] == c["pc"].shape[0] else c["rows"]
    return c


def test_library_exports_the_segloss_entry_points():
    import ctypes as C
    from nvfi_amd import _lib
    from nvfi_amd.build import build
    build()
    L = C.CDLL(_lib.SO)
    for n in ("nvfi_segloss_workspace_bytes", "nvfi_knn_self", "nvfi_segloss"):
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    assert _lib.lib().nvfi_abi_version() == 5
    nbytes = C.c_int64(0)
    assert L.nvfi_segloss_workspace_bytes(C.c_int64(9000), C.c_int(8), C.c_int(4), C.byref(nbytes)) == 0 and 0 < nbytes.value < (1 << 22)
    assert L.nvfi_segloss_workspace_bytes(C.c_int64(9000), C.c_int(17), C.c_int(4), C.byref(nbytes)) != 0          # 2 <= K <= 16
    assert b"objects" in _lib.lib().nvfi_last_error()


def test_seg_loss_module_has_the_reference_signatures():
    from nvfi_amd.utils import seg_loss
    want = {"fit_motion_svd_batch": "(pc1, pc2, mask=None)", "dynamic_loss": "(pc, mask, flow)",
            "smooth_loss": "(pc, mask, k=16, radius=0.1, loss_norm=1)", "entropy_loss": "(mask, epsilon=1e-05)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(seg_loss, name))) == sig, name
    p = list(inspect.signature(seg_loss.segm_losses).parameters)
    assert p[:7] == ["pc", "mask", "flow", "k", "radius", "smooth_w", "entropy_w"]
    assert inspect.signature(seg_loss.segm_losses).parameters["entropy_w"].default == 0
    assert not hasattr(seg_loss, "rank_loss")


def test_seg_loss_refuses_cpu_tensors():
    from nvfi_amd._lib import NvfiError
    from nvfi_amd.utils import seg_loss
    pc, flow, mask = torch.rand(1, 16, 3), torch.rand(1, 16, 3) * 0.01, torch.softmax(torch.rand(1, 16, 8), -1)
    with pytest.raises(NvfiError):
        seg_loss.dynamic_loss(pc, mask, flow)
    with pytest.raises(NvfiError):
        seg_loss.smooth_loss(pc, mask, k=4, radius=0.01)
    with pytest.raises(NvfiError):
        seg_loss.entropy_loss(mask)
    with pytest.raises(NvfiError):
        seg_loss.fit_motion_svd_batch(pc, pc + flow)
    with pytest.raises(NvfiError):
        seg_loss.segm_losses(pc, mask, flow, 4, 0.01, 0.1)


def test_segloss_source_keeps_the_rules_of_the_unit():
    """text only: no memset node (every clear is a kernel), no float atomic on the gradient, nothing that waits for the device"""
    src = open(os.path.join(ROOT, "nvfi_amd", "csrc", "segloss.hip")).read()
    for word in ("hipMemset", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "atomicAdd(a.gmask", "hipMalloc"):
        assert word not in src, word
    assert "segloss.hip" in open(os.path.join(ROOT, "nvfi_amd", "build.py")).read()


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_the_reference_goldens(sgold, name):
    c = load_case(sgold, name)
    N, K = c["mask"].shape
    rows = c["rows"]
    yidx, _, _ = s64.knn_brute(c["pc"], c["k"], c["radius"])
    differ, outside = s64.idx_mismatch(c["pc"], c["radius"], yidx[c["idx_rows"]], c["idx"], float(sgold["band"]), points=c["idx_rows"])
    print(f"[segloss64] {name}: neighbour tables differ on {differ} of {len(c['idx_rows'])} stored rows ({outside} outside the band)")
    assert outside == 0 and differ <= 5e-3 * N
    if name == "lattice_k4":
        assert np.array_equal(yidx, c["idx"])
    y = s64.segloss64(c["pc"], c["flow"], c["mask"], yidx, c["loss_norm"], 1e-5)
    y32 = s64.segloss64(c["pc"], c["flow"], c["mask"], yidx, c["loss_norm"], 1e-5, dtype=np.float32)
    err = {q: abs(y[q] - c["losses"][i]) / abs(c["losses"][i]) for i, q in enumerate(("dynamic", "smooth", "entropy"))}
    for q in ("pc_transformed", "g_dynamic", "g_smooth", "g_entropy"):
        err[q] = max(maxrel(y[q][rows], c[q]), rel_l2(y[q][rows], c[q]))
    ok = c["sv_ok"]
    assert ok.sum() >= K - 1 and np.all(np.nan_to_num(y["sv"][:, 2] / y["sv"][:, 0], nan=0.0)[ok] > float(sgold["sv_floor"]))
    err["R"] = np.abs(y["R"][ok] - c["R"][ok]).max()
    err["t"] = np.abs(y["t"][ok] - c["t"][ok]).max()
    e32 = {q: (abs(y32[q] - y[q]) / abs(y[q]) if np.ndim(y[q]) == 0 else max(maxrel(y32[q], y[q]), rel_l2(y32[q], y[q])))
           for q in ("dynamic", "smooth", "entropy", "pc_transformed", "g_dynamic", "g_smooth", "g_entropy")}
    print(f"[segloss64] {name}: against the fp32 golden " + ", ".join(f"{q} {e:.2e}" for q, e in err.items()))
    print(f"[segloss64] {name}: float32 evaluation against float64 " + ", ".join(f"{q} {e:.2e}" for q, e in e32.items()))
    for q, e in err.items():
        assert e <= BOUND[q], (name, q, e)
    if name == "zerocol":       # the all-zero column: NaN moments -> the identity, in the reference and in the yardstick
        assert not ok[2] and np.array_equal(c["R"][2], np.eye(3)) and np.array_equal(y["R"][2], np.eye(3)) and not y["t"][2].any()


def test_yardstick_gradients_are_the_derivatives_of_its_losses(sgold):
    """central differences in float64 on the small case: smoothness and entropy exactly; the dynamic loss with the fit held fixed (it is detached)"""
    c = load_case(sgold, "small")
    idx, _, _ = s64.knn_brute(c["pc"], c["k"], c["radius"])
    for norm in (1, 2):
        y = s64.segloss64(c["pc"], c["flow"], c["mask"], idx, norm, 1e-5)
        rng = np.random.default_rng(norm)
        m = c["mask"].astype(np.float64)
        d = rng.standard_normal(m.shape)
        h = 1e-8        # below the smallest non-zero |mask difference| of the case (1.7e-7): no kink of the 1-norm inside the step

        def f(mm, q):
            # float64 masks go through the same statements (the yardstick casts fp32 inputs; here the input is already float64)
            p, p2 = c["pc"].astype(np.float64), (c["pc"] + c["flow"]).astype(np.float64)
            if q == "entropy":
                return -(mm * np.log(np.maximum(mm, 1e-5))).sum(-1).mean()
            if q == "smooth":
                diff = mm[:, None, :] - mm[idx]
                return (np.abs(diff).sum(-1) if norm == 1 else np.sqrt((diff * diff).sum(-1))).mean()
            T = np.einsum("kij,nj->kni", y["R"], p) + y["t"][:, None, :]
            return np.sqrt((((mm.T[:, :, None] * T).sum(0) - p2) ** 2).sum(-1)).mean()

        for q in ("dynamic", "smooth", "entropy"):
            num = (f(m + h * d, q) - f(m - h * d, q)) / (2 * h)
            ana = float((y["g_" + q] * d).sum())
            assert abs(num - ana) <= 5e-6 * max(abs(ana), 1e-3), (q, norm, num, ana)      # (rounding of f over h: 1e-16 / 1e-8)
