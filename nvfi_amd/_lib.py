"""ctypes binding of libnvfi_hip.so (include/nvfi_hip.h).  The product path has NO CPU fallback:
a missing library or a non-GPU tensor raises."""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("NVFI_LIB", os.path.join(HERE, "csrc", "libnvfi_hip.so"))   # NVFI_LIB: alternative build (experiments)
fp = C.c_void_p

NVFI_TRAIN, NVFI_WHITE_BG, NVFI_TRANSFER, NVFI_WANT_MASK, NVFI_BWD_FORK, NVFI_WANT_FLOW, NVFI_WANT_SELECT = 1, 2, 4, 8, 16, 32, 64
NCOUNTERS = 8
NVFI_DEPTH_SKIP_HOLES = 1
NVFI_FLOWLOSS_ADD_GW = 1
NVFI_MASKLOSS_ADD_GW = 1
NVFI_DEPTH_LDS_MAX = 16384      # nvfi_depth_loss keeps both maps in LDS up to this many entries (include/nvfi_hip.h)


class FieldDesc(C.Structure):
    _fields_ = [
        ("G", C.c_int32 * 3), ("K", C.c_int32), ("Cd", C.c_int32), ("Ca", C.c_int32), ("app_dim", C.c_int32),
        ("n_samples", C.c_int32), ("use_vel", C.c_int32), ("gate_sur", C.c_int32), ("has_amask", C.c_int32), ("shading", C.c_int32), ("vel_fp16", C.c_int32),
        ("am_dims", C.c_int32 * 3),
        ("aabb", C.c_float * 6), ("near_", C.c_float), ("far_", C.c_float), ("step_size", C.c_float),
        ("density_shift", C.c_float), ("distance_scale", C.c_float), ("weight_thres", C.c_float),
        ("alpha_thres", C.c_float), ("tmax", C.c_float),
        ("gate_lo", C.c_float * 3), ("gate_hi", C.c_float * 3),
        ("dps", fp * 3), ("dpt", fp * 3), ("aps", fp * 3), ("apt", fp * 3),
        ("basis", fp), ("rW", fp * 3), ("rb", fp * 3),
        ("vW", fp * 6), ("vb", fp * 6), ("aW", fp * 6), ("ab", fp * 6),
        ("amask", fp),
        ("frags", fp),
    ]


class MaskDesc(C.Structure):
    _fields_ = [("n_layer", C.c_int32), ("n_dim", C.c_int32), ("mask_dim", C.c_int32), ("W", fp * 5), ("b", fp * 5)]


class AdamTensor(C.Structure):
    _fields_ = [("p", fp), ("g", fp), ("m", fp), ("v", fp), ("n", C.c_int64), ("lr", C.c_float)]


class MaskGrads(C.Structure):
    _fields_ = [("W", fp * 5), ("b", fp * 5)]


class Grads(C.Structure):
    _fields_ = [
        ("dps", fp * 3), ("dpt", fp * 3), ("aps", fp * 3), ("apt", fp * 3),
        ("basis", fp), ("rW", fp * 3), ("rb", fp * 3),
        ("vW", fp * 6), ("vb", fp * 6), ("aW", fp * 6), ("ab", fp * 6),
    ]


class DrawDesc(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("iteration", C.c_uint64), ("iteration_dev", fp),
                ("n_batches", C.c_int32), ("R", C.c_int64), ("n_pixels", C.c_int64),
                ("bundle_o", fp), ("bundle_d", fp), ("target_img", fp),
                ("rays_o", fp * 2), ("rays_d", fp * 2), ("target", fp * 2), ("pixel_ids", fp * 2),
                ("P", C.c_int64), ("aabb", C.c_float * 6), ("points", fp), ("t", fp)]


# The prototypes of include/nvfi_hip.h, one row per function in the header's order: a letter per parameter - p any pointer (a struct by
# reference, a device pointer, a stream, NULL), l int64_t, i int, f float.  lib() turns every row into argtypes, so a call site passes plain
# Python numbers and a wrong kind is refused before the call is made; tests/test_abi_and_host.py holds the table against the header.
ABI_VERSION = 5
KINDS = {"p": C.c_void_p, "l": C.c_int64, "i": C.c_int, "f": C.c_float}
SIGNATURES = {
    "nvfi_last_error": "",      # returns const char*; every other function an int error code
    "nvfi_abi_version": "",
    "nvfi_render_workspace_bytes": "plip",
    "nvfi_render_workspace_bytes_t": "plifp",
    "nvfi_render_fwd": "plpppfippppplpp",
    "nvfi_render_bwd": "plppfippppppplp",
    "nvfi_render_fwd_t": "plpppfpippppplpp",
    "nvfi_render_bwd_t": "plppfiippppppplp",
    "nvfi_render_fwd_mse": "plpppfpippppplppfppp",
    "nvfi_frag_cache_bytes": "pp",
    "nvfi_pack_frags": "pplp",
    "nvfi_stream_capture_id": "pp",
    "nvfi_pde_workspace_bytes": "plp",
    "nvfi_pde_loss": "plppfppplpp",
    "nvfi_pde_loss_ex": "plppfppplppplpp",
    "nvfi_pde_loss_split": "plppfppplppplppp",
    "nvfi_pde_loss_dev": "plpppppplpp",
    "nvfi_render_mask": "pplfippplp",
    "nvfi_render_export_masked": "plfipllppp",
    "nvfi_render_flow": "plppffippiifpppplp",
    "nvfi_render_objects": "pplfippppplp",
    "nvfi_render_fwd_select": "ppplpppfippppplpp",
    "nvfi_maskfield_workspace_bytes": "plip",
    "nvfi_maskfield_fwd": "plppiplp",
    "nvfi_maskfield_bwd": "plppiplp",
    "nvfi_segloss_workspace_bytes": "liip",
    "nvfi_knn_self": "lpifppppplp",
    "nvfi_segloss": "lipppipppifffffipppppplp",
    "nvfi_char_workspace_bytes": "plp",
    "nvfi_char_loss": "plpffpppplp",
    "nvfi_sh_render": "lpppp",
    "nvfi_plane_regs": "pfffppp",
    "nvfi_plane_regs_dev": "ppppp",
    "nvfi_mse": "pplppp",
    "nvfi_depth_loss": "lpppifpppp",
    "nvfi_ray_distortion_workspace_bytes": "lp",
    "nvfi_ray_distortion": "lipffppppplp",
    "nvfi_flow_loss_workspace_bytes": "plfflp",
    "nvfi_flow_loss_fwd": "plppffippiifppiffpippppllplp",
    "nvfi_flow_loss_bwd": "plffllpplp",
    "nvfi_mask_loss_workspace_bytes": "ppllp",
    "nvfi_mask_loss_fwd": "pplfipppiffpippppllplp",
    "nvfi_mask_loss_bwd": "plillpplp",
    "nvfi_adam_step": "piffflip",
    "nvfi_adam_step_dev": "pifffpip",
    "nvfi_vel_eval": "plppiplp",
    "nvfi_vel_workspace_bytes": "plp",
    "nvfi_integrate_pos": "plppppplp",
    "nvfi_advect_grad_workspace_bytes": "plffp",
    "nvfi_advect_grad": "plpffpppplp",
    "nvfi_density_at": "plpppp",
    "nvfi_app_workspace_bytes": "plp",
    "nvfi_app_at": "plpppplp",
    "nvfi_density_grad": "plppppp",
    "nvfi_appfeat_at": "plppp",
    "nvfi_appfeat_grad": "plppppp",
    "nvfi_render_mlp": "plppppplp",
    "nvfi_render_mlp_grad_workspace_bytes": "plp",
    "nvfi_render_mlp_grad": "plppppppppplp",
    "nvfi_comm_unique_id": "p",
    "nvfi_comm_init": "piip",
    "nvfi_allreduce_grads": "pplip",
    "nvfi_comm_destroy": "p",
    "nvfi_prof_enable": "i",
    "nvfi_prof_collect": "pp",
    "nvfi_prof_nclasses": "",
    "nvfi_alpha_workspace_bytes": "plp",
    "nvfi_compute_alpha": "plpfifipplp",
    "nvfi_gen_rays": "piiflpppp",
    "nvfi_draw_batch": "pp",
    "nvfi_metrics_workspace_bytes": "iliiip",
    "nvfi_ssim": "liiipppppfipplp",
    "nvfi_segm_confusion": "lliippppppplp",
    "nvfi_debug_act": "ilppp",
    "nvfi_selftest": "pp",
}
EXPORTS = list(SIGNATURES)
# The prototypes of the headers include/nvfi_hip.h brings in behind its own list, same letters: header -> rows in the header's order.  lib() binds
# them exactly like SIGNATURES; tests/test_advect_pt_abi.py holds the rows against include/nvfi_hip_advect_pt.h.
ADDITIONS = {
    "nvfi_hip_advect_pt.h": {
        "nvfi_advect_pt_steps": "plppppp",
        "nvfi_advect_grad_pt_workspace_bytes": "plip",
        "nvfi_advect_grad_pt": "plpppippppplp",
    },
}

_LIB = None


class NvfiError(RuntimeError):
    pass


def lib():
    """Load the HIP library; fail loudly if it has not been built (no fallback path exists)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO):
            raise NvfiError(f"{SO} is missing: build it with `python -m nvfi_amd.build` (needs hipcc). "
                            "There is no CPU fallback for the NVFi hot path.")
        L = C.CDLL(SO)
        for table in [SIGNATURES] + list(ADDITIONS.values()):
            for name, kinds in table.items():       # getattr raises AttributeError on a missing symbol
                getattr(L, name).argtypes = [KINDS[k] for k in kinds]
        L.nvfi_last_error.restype = C.c_char_p      # every other function returns int, ctypes' default
        if L.nvfi_abi_version() != ABI_VERSION:
            raise NvfiError(f"{SO} has ABI version {L.nvfi_abi_version()}, this binding is written for {ABI_VERSION}: rebuild it "
                            "with `python -m nvfi_amd.build` (or unset NVFI_LIB)")
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise NvfiError(f"libnvfi_hip error {rc}: {lib().nvfi_last_error().decode()}")


def bytes_of(fn, *args):
    """the int64 a size query of the library (nvfi_*_bytes) answers through its last argument"""
    nb = C.c_int64(0)
    check(fn(*args, C.byref(nb)))
    return nb.value


def capture_id(stream_handle):
    """id (> 0) of the hipGraph capture the stream takes part in, 0 when it is not capturing"""
    cid = C.c_uint64(0)
    check(lib().nvfi_stream_capture_id(stream_handle, C.byref(cid)))
    return cid.value


def ptr(t):
    """Device pointer of a torch tensor (or NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    """handle of torch's current stream, as the `stream` argument of every library call"""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def plan_chunks(nbytes_of, cap, max_workspace_bytes, what, unit="entry"):
    """(chunk, bytes, chunks) of a stash-bound adjoint over `cap` entries whose workspace for n entries at a time is nbytes_of(n): everything
    at once when that fits max_workspace_bytes, else the largest multiple of 128 whose plan fits - found from an affine guess through the 128
    and the 256 plan (the plans grow by whole 128-entry groups), stepped down while too large.  One group that does not fit is refused."""
    chunk = cap
    if nbytes_of(cap) > max_workspace_bytes:
        b1, b2 = nbytes_of(128), nbytes_of(256)
        if b1 > max_workspace_bytes:
            raise NvfiError(f"{what}: max_workspace_bytes={max_workspace_bytes} is below the {b1} bytes one 128-{unit} group needs")
        chunk = 128 * (1 + (max_workspace_bytes - b1) // max(b2 - b1, 1))
        while chunk > 128 and nbytes_of(chunk) > max_workspace_bytes:
            chunk -= 128
        chunk = min(chunk, cap)
    return chunk, nbytes_of(chunk), (cap + chunk - 1) // chunk if cap else 0
