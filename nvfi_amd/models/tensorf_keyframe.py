"""TensorVMKeyframeTimeKplane - host-side mirror of the reference field module
(models/tensorf_keyframe.py:37-756 + models/tensorf_base.py:133-269) for the render hot path.

Parameters keep the reference's names and logical shapes (state_dict compatible, including the
duplicated `vel.vel_net.*` keys, tensorf_keyframe.py:94,106); the factor planes are stored
physically channel-last so one bilinear tap is one contiguous vector for the HIP kernels.
Everything between "rays in" and "rgb/depth/acc/weights (+ gradients) out" is one call into
libnvfi_hip.so through ctypes; there is no PyTorch/CPU fallback.
"""
import ctypes as C
import os
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._lib import stream_ptr as _stream_ptr
from . import field_slots as fs
from .field_autograd import _AdvectFn, _AdvectPtFn, _AppLookupFn, _CharFn, _DensityLookupFn, _FlowLossFn, _MaskLossFn, _PdeFn, _RegFn, _RenderFn, _ShadeFn
from .field_grads import FieldGrads, _rt, round64
from .mask_field import _mask_desc
from .tensorf_model_utils import AlphaGridMask
from .velocity_field import VelBasis, VelocityAABB, VelocityAABBSur

# render_mse_backward_: the slots of the 64-float `loss` piece of its output buffer, one owner each
_LOSS_MSE = 0                  # nvfi_render_fwd_mse
_LOSS_DEPTH = 1                # nvfi_depth_loss: the value ...
_LOSS_DEPTH_COUNT = 2          # ... and its int64 count of the entries that took part (8-byte aligned: two floats)
_LOSS_DISTORTION = 4           # nvfi_ray_distortion
_LOSS_FLOW = 6                 # nvfi_flow_loss_fwd: the value and, in the next slot, n (the number of rays that counted)
_LOSS_MASK = 8                 # nvfi_mask_loss_fwd: the value and, in the next slot, n (the number of rays that are not ignored)


class MLPRender_PE(nn.Module):
    """Parameter container of the appearance decoder (tensorf_base.py:67-98); evaluated by k_app_fwd."""

    def __init__(self, inChanel, viewpe=6, pospe=6, featureC=128):
        super().__init__()
        self.in_mlpC = (3 + 2 * viewpe * 3) + (3 + 2 * pospe * 3) + inChanel
        self.viewpe, self.pospe = viewpe, pospe
        self.mlp = nn.Sequential(nn.Linear(self.in_mlpC, featureC), nn.ReLU(inplace=True),
                                 nn.Linear(featureC, featureC), nn.ReLU(inplace=True), nn.Linear(featureC, 3))
        nn.init.constant_(self.mlp[-1].bias, 0)
        self._owner = None

    def forward(self, pts, viewdirs, features, kwargs=None):
        """renderModule(pts, viewdirs, features) as the reference's module can be called (tensorf_base.py:88-98): the positional encodings and
        the MLP of the fused appearance kernel on the caller's features (nvfi_render_mlp).  Forward only - inside a render the module is
        differentiated by nvfi_render_bwd; a stand-alone call that needs gradients is refused rather than silently detached."""
        field = self._owner() if callable(self._owner) else self._owner
        if field is None:
            raise _lib.NvfiError("MLPRender_PE.forward needs the field it belongs to (it is created by TensorVMKeyframeTimeKplane)")
        if torch.is_grad_enabled() and (features.requires_grad or pts.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("stand-alone MLPRender_PE.forward is forward-only: call it under torch.no_grad() "
                                      "(gradients of the render module flow through Renderer.render / NVFi.render_ray; "
                                      "at given points, through field.shade / field.lookup_rgb)")
        return field._render_module_call(pts, viewdirs, features)


def SHRender(xyz_sampled, viewdirs, features, kwargs=None):
    """tensorf_model_utils.py:292-296 as a stand-alone call (inside a render it is fused into k_app_fwd / k_app_bwd)."""
    return TensorVMKeyframeTimeKplane.sh_render(viewdirs, features)


class DeviceTime(float):
    """A frame time whose VALUE lives in device memory: `DeviceTime(t_plan, dev)` is a float (t_plan - it fixes the launch plan: keyframe or
    not, number of RK2 steps, workspace layout) that carries a 1-element fp32 CUDA tensor `dev` the kernels read the time from
    (nvfi_render_fwd_t).  Passing it as `t` to Renderer.render / NVFi.render_ray lets a captured hipGraph of a training iteration be
    replayed with a new time every iteration.  dev[0] must be in the same plan class as t_plan (counters[7] reports a mismatch)."""

    def __new__(cls, t_plan, dev):
        x = super().__new__(cls, float(t_plan))
        if not (isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and dev.numel() == 1):
            raise _lib.NvfiError("DeviceTime needs a 1-element fp32 CUDA tensor")
        x.dev = dev
        return x


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


class TensorVMKeyframeTimeKplane(FieldGrads, nn.Module):
    def __init__(self, aabb, gridSize, device, near_far, cfg):
        super().__init__()
        self.matModeSpace = [[0, 1], [0, 2], [1, 2]]
        self.matModeTime = [[2, 3], [1, 3], [0, 3]]
        self.cfg = cfg
        self.device = device
        self.num_keyframes = cfg.num_keyframes
        self.tmax = cfg.tmax
        self.time_scale_factor = self.tmax / (self.num_keyframes - 1) if self.num_keyframes > 1 else 1
        self.densityMode = cfg.densityMode
        if self.densityMode != "Density":
            raise NotImplementedError("only densityMode=Density is on the hot path (every shipped config)")
        self.data_dim_density = 1
        self.register_buffer("aabb", aabb.to(device).float())
        self.step_ratio = cfg.step_ratio
        self.max_n_samples = cfg.max_n_samples
        self.near_far = near_far
        self.density_n_comp = cfg.density_n_comp
        self.app_n_comp = cfg.appearance_n_comp
        self.app_dim = cfg.app_dim
        self.density_shift = cfg.density_shift
        self.distance_scale = cfg.distance_scale
        self.alphaMask = None
        self.alphaMask_thres = cfg.alphaMask_thres
        self.rayMarch_weight_thres = cfg.rayMarch_weight_thres
        self.fea2denseAct = cfg.fea2denseAct
        if self.fea2denseAct != "softplus":
            raise NotImplementedError("only fea2denseAct=softplus is on the hot path (every shipped config)")
        self.update_stepSize(gridSize)
        self.init_svd_volume(device)
        self.shadingMode = cfg.shadingMode
        self.pos_pe, self.view_pe, self.fea_pe, self.featureC = cfg.pos_pe, cfg.view_pe, cfg.fea_pe, cfg.featureC
        if self.shadingMode == "SH":
            # tensorf_base.py:196-197: renderModule is the FUNCTION SHRender (no parameters); basis_mat maps the 48 plane products to 27 SH coefficients
            if self.app_dim != 27:
                raise NotImplementedError("shadingMode=SH needs app_dim=27 (3 colours x 9 degree-2 SH coefficients)")
            self.renderModule = SHRender
        elif self.shadingMode == "MLP_PE":
            if self.pos_pe != 6 or self.view_pe != 6 or self.featureC != 128 or self.app_dim != 32:
                raise NotImplementedError("shadingMode=MLP_PE is built for pos_pe=view_pe=6, featureC=128, app_dim=32 (every shipped config)")
            self.renderModule = MLPRender_PE(self.app_dim, self.view_pe, self.pos_pe, self.featureC).to(device)
            self.renderModule._owner = weakref.ref(self)      # renderModule(pts, viewdirs, features) evaluates on this field's kernels
        else:
            raise NotImplementedError("shadingMode must be MLP_PE or SH (MLP_Fea / MLP / RGB* are not on the hot path: no shipped config uses them)")
        self.use_vel = bool(cfg.use_vel)
        if self.use_vel:
            self.vel_net = VelBasis().to(device)
            self.vel_net._owner = weakref.ref(self)
            eps = cfg.eps if "eps" in cfg else 0.03
            if all(k in cfg for k in ("sur_x", "sur_y", "sur_z")):
                sur = torch.stack([torch.tensor(cfg[k]) for k in ("sur_x", "sur_y", "sur_z")], dim=-1).to(device)
                self.vel = VelocityAABBSur(self.vel_net, self.aabb.clone(), sur)
            else:
                self.vel = VelocityAABB(self.vel_net, eps)
        self.mask_field = None
        self.contract_ray = bool("contract_ray" in cfg and cfg.contract_ray)
        if self.contract_ray:
            raise NotImplementedError("contract_ray is out of scope")
        self.last_counters = None
        # Where the backward kernels put parameter gradients:
        #   False (default)    pure autograd: gradients are returned to the engine - torch.autograd.grad(), parameter hooks and
        #                      post-accumulate-grad hooks (DDP, optimiser-in-backward, clipping hooks) behave as for any nn.Module
        #   "arena" (opt-in: NVFI_INPLACE_GRADS=arena, field.accumulate_grads_inplace = "arena"; bench.py --mode dropin and
        #                      tools/run_reference_driver.py switch it on) straight into p.grad, which the field backs with ONE persistent
        #                      flat buffer that it zeroes once per iteration (when the driver's zero_grad(set_to_none=True) left every
        #                      .grad None): no fresh 38 MB gradient tensors and no AccumulateGrad add per parameter and backward node.
        #                      p.grad tensors are then re-used across iterations (aliasing: keep a .clone() if you need last iteration's
        #                      values) and the engine is handed None for the parameters; a field with ANY autograd hook on a parameter
        #                      falls back to pure autograd for that call
        #   True               same, but the caller owns p.grad (nvfi_amd.dist.GradBucket: every .grad is a view of its flat buffer)
        self.accumulate_grads_inplace = "arena" if os.environ.get("NVFI_INPLACE_GRADS", "0") in ("1", "arena") else False
        # Opt-in (NVFI_AUTO_OVERLAP=1): train-mode render / PDE calls run on the field's own side streams (the caller's stream waits for
        # the results), so that the chains of an iteration - and their backward passes, which autograd runs on the stream of the forward -
        # can overlap on the device under a sequential driver.  MEASURED SLOWER under the reference's loop (bench.py --mode dropin:
        # 372-438 k rays/s against 481 k on one stream): that loop waits for the device three times per iteration, so it is bound by the
        # host's issue time between the waits, and the extra cross-stream waits / record_stream bookkeeping only add to it.  Off by default.
        self.auto_overlap = os.environ.get("NVFI_AUTO_OVERLAP", "0") == "1"
        self.pde_debug = 0   # >0: also return the kept mask and the first n Jacobians of get_vel_loss
        # the backward of a keyframe render may run its density half beside its appearance half on a library-owned stream (NVFI_BWD_FORK);
        # a driver that already overlaps renders / the PDE term on its own streams (bench.py's fused step) switches this off
        self.fork_backward = os.environ.get("NVFI_BWD_FORK", "1") != "0"
        self.pde_split = os.environ.get("NVFI_PDE_SPLIT", "1") != "0"     # pde_loss(): adjoint half of the call on a side stream (nvfi_pde_loss_split)
        # opt-in (not a reference attribute; the reference's counterpart is autocast via --disable_fp32, train_nvfi.py:96,144): every no-grad
        # back-advection - integrate_pos, the warp of eval-mode renders, getDenseAlpha - on the fp16-input MFMA (nvfi_field_desc.vel_fp16).
        # Training renders, the PDE term and all gradients stay fp32 whatever this says.
        # True / 1: one binary16 term per MFMA operand; 2 / "split": two terms (fp32 products emulated, ~2^-21 relative per product, 2.4x fp32 speed)
        self.vel_fp16 = {"0": False, "1": True, "2": 2, "split": 2, "3": 3, "x6": 3}.get(os.environ.get("NVFI_VEL_FP16", "0"), False)
        # opt-in (round 4; the reference's counterpart: --disable_fp32 autocasts the forward of every nn.Linear, train_nvfi.py:96,144): the velocity
        # warp of TRAINING renders evaluates VelBasis forward with fp16-input MFMAs (fp32 accumulation, fp32 stashes); its adjoint and the
        # weight gradients stay fp32 MFMA on those stashes, the PDE term and the render MLP stay fp32.  Never the default, never the headline.
        self.vel_fp16_train = os.environ.get("NVFI_VEL_FP16_TRAIN", "0") == "1"
        self.register_load_state_dict_post_hook(lambda m, k: m.update_stepSize(m.gridSize.tolist()))

    # ------------------------------------------------------------------ construction
    def update_stepSize(self, gridSize):
        """tensorf_base.py:214-227"""
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invaabbSize = 2.0 / self.aabbSize
        self.gridSize = torch.LongTensor([int(g) for g in gridSize]).to(self.aabb.device)
        self.units = self.aabbSize / (self.gridSize - 1)
        self.stepSize = torch.mean(self.units) * self.step_ratio
        self.aabbDiag = torch.sqrt(torch.sum(torch.square(self.aabbSize)))
        self.nSamples = min(self.max_n_samples, int((self.aabbDiag / self.stepSize).item()) + 1)
        # host copies of the scalars the C ABI needs (no device sync per render call)
        self._aabb_host = [float(v) for v in self.aabb.detach().reshape(-1).cpu().tolist()]
        self._grid_host = [int(g) for g in gridSize]
        self._step_host = float(self.stepSize)

    def _init_planes(self, n_component, gridSize, numFrames, scale, device):
        """tensorf_keyframe.py:136-186 (softplus branch): uniform(0.1,0.5)*scale space planes, ones time planes."""
        space, time = [], []
        for i in range(3):
            a, b = self.matModeSpace[i]
            c = self.matModeTime[i][0]
            p = torch.empty(1, n_component[i], int(gridSize[b]), int(gridSize[a]))
            nn.init.uniform_(p, a=0.1, b=0.5)
            space.append(nn.Parameter(_cl(scale * p)))
            time.append(nn.Parameter(_cl(torch.ones(1, n_component[i], numFrames, int(gridSize[c])))))
        return nn.ParameterList(space).to(device), nn.ParameterList(time).to(device)

    def init_svd_volume(self, device):
        gs = self.gridSize.tolist()
        self.density_plane_space, self.density_plane_time = self._init_planes(self.density_n_comp, gs, self.num_keyframes, 0.8, device)
        self.app_plane_space, self.app_plane_time = self._init_planes(self.app_n_comp, gs, self.num_keyframes, 0.1, device)
        self.basis_mat = nn.Linear(self.app_n_comp[0], self.app_dim, bias=False).to(device)
        self.basis_mat_density = nn.Linear(self.density_n_comp[0], self.data_dim_density, bias=False).to(device)
        self._fix_layout()

    def _fix_layout(self):
        for pl in (self.density_plane_space, self.density_plane_time, self.app_plane_space, self.app_plane_time):
            for p in pl:
                if not p.data.is_contiguous(memory_format=torch.channels_last):
                    p.data = _cl(p.data)

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        _rt(self).pop("_rp_cache", None); _rt(self).pop("_pp_cache", None)
        self._fix_layout()
        self.device = self.aabb.device
        for name in ("gridSize", "aabbSize", "invaabbSize", "units", "stepSize", "aabbDiag"):
            if hasattr(self, name) and isinstance(getattr(self, name), torch.Tensor):
                setattr(self, name, getattr(self, name).to(self.aabb.device))
        if self.use_vel and isinstance(self.vel, VelocityAABBSur):
            self.vel.bounds = self.vel.bounds.to(self.aabb.device)
        return r

    # ------------------------------------------------------------------ parameter plumbing
    def _param_key(self):
        d = self.__dict__["_modules"]
        lists = (d["density_plane_space"], d["density_plane_time"], d["app_plane_space"], d["app_plane_time"])
        return tuple(id(p) for pl in lists for p in pl._parameters.values()) + (self.use_vel, self.shadingMode, id(d.get("vel_net")), id(d.get("renderModule")))

    def _render_params(self):
        """The 31 tensors of the render path in nvfi_field_desc order.  Walking the module tree costs ~90 us of host time per call (and a
        step makes seven of them), so the list is cached and re-validated by the identities of the plane parameters / sub-modules
        (shrink / upsample_volume_grid replace them; `.to()` keeps them)."""
        key = self._param_key()
        c = _rt(self).get("_rp_cache")
        if c is not None and c[0] == key:
            return list(c[1])
        ps = self._render_params_walk()
        _rt(self)["_rp_cache"] = (key, tuple(ps))
        return ps

    def _render_params_walk(self):
        ps = list(self.density_plane_space) + list(self.density_plane_time) + list(self.app_plane_space) + list(self.app_plane_time)
        ps.append(self.basis_mat.weight)
        if self.shadingMode == "SH":
            ps += [None] * (fs.RENDER_MLP.stop - fs.RENDER_MLP.start)      # no render MLP: the six slots stay empty so that the velocity slots keep their index
        else:
            for i in (0, 2, 4):
                ps += [self.renderModule.mlp[i].weight, self.renderModule.mlp[i].bias]
        if self.use_vel:
            for lin in VelBasis.linears(self.vel_net.weight_net):
                ps += [lin.weight, lin.bias]
        return ps

    def _pde_params(self):
        c = _rt(self).get("_pp_cache")
        vn = self.__dict__["_modules"].get("vel_net")
        if c is not None and c[0] == id(vn):
            return list(c[1])
        ps = self._pde_params_walk()
        _rt(self)["_pp_cache"] = (id(vn), tuple(ps))
        return ps

    def _pde_params_walk(self):
        ps = []
        for net in (self.vel_net.weight_net, self.vel_net.a_weight_net):
            for lin in VelBasis.linears(net):
                ps += [lin.weight, lin.bias]
        return ps

    def _gate(self):
        if not self.use_vel:
            return 0, [-1.0] * 3, [1.0] * 3
        if isinstance(self.vel, VelocityAABBSur):
            if getattr(self, "_sur_host", None) is None:
                b = self.vel.bounds.detach().float().cpu().numpy()
                self._sur_host = (b[0].tolist(), b[1].tolist())
            return 1, self._sur_host[0], self._sur_host[1]
        eps = float(self.vel.eps)
        return 0, [float(np.float32(-1 + eps))] * 3, [float(np.float32(1 - eps))] * 3

    def __deepcopy__(self, memo):
        """a copy's sub-modules (vel_net, renderModule) must evaluate on the COPY's kernels / descriptor, not on the original's:
        the weak back-references are re-pointed after the default deep copy"""
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        for child in (getattr(new, "vel_net", None), getattr(new, "renderModule", None)):
            if isinstance(child, nn.Module) and "_owner" in child.__dict__:
                child.__dict__["_owner"] = weakref.ref(new)
        return new

    def _host_state(self):
        """every host-side attribute nvfi_field_desc's scalar fields are derived from (attributes a caller may assign at any time)"""
        am = self.alphaMask
        vel = self.__dict__["_modules"].get("vel") if self.use_vel else None
        return (self.nSamples, self._step_host, tuple(self._aabb_host), tuple(self._grid_host), self.num_keyframes, self.use_vel, self.shadingMode,
                self.vel_fp16, self.__dict__.get("vel_fp16_train", False), self.density_shift, self.distance_scale, self.rayMarch_weight_thres,
                self.alphaMask_thres, self.tmax, self.near_far[0], self.near_far[1], self.app_dim,
                0 if am is None else am.alpha_volume.data_ptr(), id(vel), getattr(vel, "eps", None) if vel is not None else None)

    def _desc(self, params=None):
        """nvfi_field_desc for the current parameters (or for the tensors saved by autograd).  Building the ctypes struct costs ~25 us of
        host time and a training iteration makes eight of them, so the struct is cached and re-validated by the parameters' device
        pointers and the host attributes it is derived from; the caller gets a private copy (the backward edits vel_fp16).  `frags`
        (ABI v5) points at the field's fragment cache when that is current for these weights (_frags)."""
        ps = self._render_params() if params is None else list(params)
        pp = self._pde_params() if self.use_vel else []
        key = (tuple(0 if p is None else p.data_ptr() for p in ps), tuple(p.data_ptr() for p in pp[fs.PDE_A_WEIGHT_NET]), self._host_state())
        rt = _rt(self)
        c = rt.get("_desc_cache")
        if c is None or c[0] != key:
            c = (key, self._desc_build(ps, pp))
            rt["_desc_cache"] = c
        d = _lib.FieldDesc.from_buffer_copy(c[1])
        d.frags = self._frags(d, ps, pp)
        return d

    def _desc_build(self, ps, pp):
        d = _lib.FieldDesc()
        d.G[:] = self._grid_host
        d.K = int(self.num_keyframes)
        d.Cd, d.Ca, d.app_dim = int(self.density_n_comp[0]), int(self.app_n_comp[0]), int(self.app_dim)
        d.shading = 1 if self.shadingMode == "SH" else 0
        # 3 / "x6": every no-grad back-advection on the x6 kernels (vel_x6.hip: fp32 products formed exactly from three binary16 terms per operand)
        vf = self.vel_fp16
        # "fp32" (bit 3): keep the fp32 MFMA kernels for integrate_pos / compute_alpha, whose default since round 6 is x6 too (the A/B reference)
        d.vel_fp16 = ((8 if vf == "fp32" else 3 if (vf == 3 or vf == "x6") else (2 if vf in (2, "split", "split16") else (1 if vf else 0)))
                      | (4 if getattr(self, "vel_fp16_train", False) else 0))
        d.n_samples = int(self.nSamples)
        d.use_vel = int(self.use_vel)
        gsur, lo, hi = self._gate()
        d.gate_sur = gsur
        d.gate_lo[:] = lo
        d.gate_hi[:] = hi
        d.aabb[:] = self._aabb_host
        d.near_, d.far_ = float(self.near_far[0]), float(self.near_far[1])
        d.step_size = self._step_host
        d.density_shift, d.distance_scale = float(self.density_shift), float(self.distance_scale)
        d.weight_thres, d.alpha_thres, d.tmax = float(self.rayMarch_weight_thres), float(self.alphaMask_thres), float(self.tmax)
        for p in ps[fs.FACTOR_PLANES]:
            if not p.is_contiguous(memory_format=torch.channels_last):
                raise _lib.NvfiError("factor planes must be channels_last (call field._fix_layout())")
        fs.fill(d, ps)
        if self.use_vel:
            fs.fill(d, pp, fs.PDE_A_MEMBERS)
        if self.alphaMask is not None:
            d.has_amask = 1
            v = self.alphaMask.alpha_volume
            d.am_dims[:] = [v.shape[-1], v.shape[-2], v.shape[-3]]
            d.amask = _lib.ptr(v)
        d.frags = None
        return d

    # ------------------------------------------------------------------ fragment cache (ABI v5: nvfi_pack_frags)
    def _frags(self, d, ps, pp):
        """Device pointer of the field's fragment cache, current for the weights `d` describes - or None (the call then repacks into its
        own workspace).  The cache is keyed on (data_ptr, _version) of every nn.Linear tensor it is built from plus the generation counter
        of nvfi_amd.optim.Adam (whose HIP launch does not pass through torch's version counter): the first call after an optimiser step
        repacks - ONE launch on the current stream instead of 7 across the iteration's calls - and later calls on other streams wait for
        that launch once.  An in-place edit through `.data` bumps neither: call invalidate_frags().  NVFI_FRAG_CACHE=0 switches it off."""
        rt = _rt(self)
        on = rt.get("_frag_on")
        if on is None:
            on = rt["_frag_on"] = os.environ.get("NVFI_FRAG_CACHE", "1") != "0"
        if not on or not ps[0].is_cuda:
            return None
        from .. import optim as _optim
        lin = [p for p in ps[fs.LINEARS] if p is not None] + list(pp[fs.PDE_A_WEIGHT_NET])
        key = (tuple(p.data_ptr() for p in lin), tuple(p._version for p in lin), _optim.GENERATION, rt.get("_frag_epoch", 0))
        fc = rt.get("_frag_cache")
        cur = torch.cuda.current_stream()
        # Under hipGraph capture the pointer is BAKED into the graph: a cache that is current now says nothing about the replays, which run
        # after optimiser steps the key will never see.  So while capturing, the cache is used only if its pack launch is a node
        # of THIS capture (repack_frags() at the head of the captured iteration; forked streams share the capture id) - or if the driver
        # vouches that it replays the graph holding the pack node first (frags_packed_by_earlier_graph, the three-graph multi-rank step);
        # everything else packs per call, whatever the key says.
        cap = _lib.capture_id(cur.cuda_stream) if torch.cuda.is_current_stream_capturing() else 0
        repack_now = bool(rt.get("_frag_capture_ok"))
        if cap and not repack_now and not rt.get("_frag_trust_graph"):
            if fc is None or fc["key"] != key or fc.get("capture") != cap:
                return None
        if repack_now or fc is None or fc["key"] != key or fc["buf"].device != ps[0].device:
            if cap and not repack_now:
                return None         # (a captured iteration repacks explicitly at its head: repack_frags(); anything else packs per call)
            L = _lib.lib()
            buf = fc["buf"] if fc is not None and fc["buf"].device == ps[0].device else None
            if buf is None:
                nb = _lib.bytes_of(L.nvfi_frag_cache_bytes, C.byref(d))
                buf = torch.empty(nb, dtype=torch.uint8, device=ps[0].device)
            d.frags = None
            _lib.check(L.nvfi_pack_frags(C.byref(d), _lib.ptr(buf), buf.numel(), C.c_void_p(cur.cuda_stream)))
            ev = torch.cuda.Event()
            ev.record(cur)
            fc = rt["_frag_cache"] = dict(key=key, buf=buf, event=ev, stream=cur, waited=set(), capture=cap)
            rt["_frag_capture_ok"] = False
        elif cur != fc["stream"] and cur.cuda_stream not in fc["waited"]:
            cur.wait_event(fc["event"])
            fc["waited"].add(cur.cuda_stream)
        return fc["buf"].data_ptr()

    def render_workspace_bytes(self, R, t, train=False, transfer=False, flow=False, objects=False):
        """bytes nvfi_render_fwd[_t] plans for R rays at time t (include/nvfi_hip.h: nvfi_render_workspace_bytes_t); flow: with the room
        nvfi_render_flow needs (render_flow); objects: with the mask branch's and nvfi_render_fwd_select's room (render_objects)"""
        desc = self._desc()
        flags = (_lib.NVFI_TRAIN if train else 0) | (_lib.NVFI_TRANSFER if transfer else 0) | (_lib.NVFI_WANT_FLOW if flow else 0)
        if objects:
            flags |= _lib.NVFI_WANT_MASK | _lib.NVFI_WANT_SELECT
        return _lib.bytes_of(_lib.lib().nvfi_render_workspace_bytes_t, C.byref(desc), int(R), flags, float(t))

    def invalidate_frags(self):
        """the weights were edited behind torch's version counters (p.data.copy_(), a raw kernel): the next call repacks"""
        rt = _rt(self)
        rt["_frag_epoch"] = rt.get("_frag_epoch", 0) + 1

    def repack_frags(self):
        """Repack the fragment cache NOW on the current stream (one launch) whatever its key says, and leave it current: a driver that forks
        the iteration's chains over several streams - or captures the iteration as a hipGraph - calls this at the head of the iteration.
        Under capture the pack launch becomes a node of the graph and only calls of the SAME capture read the cache (_frags)."""
        self.invalidate_frags()
        rt = _rt(self)
        rt["_frag_capture_ok"] = True
        try:
            self._desc()
        finally:
            rt["_frag_capture_ok"] = False

    def frags_packed_by_earlier_graph(self, on=True):
        """A driver that captures the iteration as SEVERAL graphs (bench.py: the multi-rank step) packs in the first and replays it before
        the others: it tells the field so for the duration of the later captures - the only case in which a captured call may read a cache
        whose pack launch is not a node of its own capture."""
        _rt(self)["_frag_trust_graph"] = bool(on)

    def _params_with(self, group, tensors):
        """the current 31-list with the slots of `group` (a slice of field_slots) replaced by `tensors`, e.g. the ones autograd saved"""
        ps, tensors = self._render_params(), list(tensors)
        if len(ps[group]) != len(tensors):
            raise ValueError(f"{len(tensors)} tensors for the {len(ps[group])} slots of {group}")
        ps[group] = tensors
        return ps

    def _grads_struct(self, grads):
        """nvfi_grads over gradient tensors in _render_params() order (a shorter list leaves NULL behind it)"""
        return fs.fill(_lib.Grads(), grads)

    def _grads_struct_vel(self, grads):
        """nvfi_grads over the 24 gradient tensors of both velocity nets, in _pde_params() order"""
        return fs.fill(_lib.Grads(), grads, fs.PDE_MEMBERS)

    # ------------------------------------------------------------------ hot path
    def _prep_rays(self, ray_o, ray_d, t):
        """the rays of a call as contiguous fp32 (R, 3) device tensors and its time as an fp32 value (no CPU fallback exists)"""
        if not ray_o.is_cuda or not self.aabb.is_cuda:
            raise _lib.NvfiError("NVFi HIP kernels need the field and the rays on the GPU (no CPU fallback exists)")
        return ray_o.reshape(-1, 3).contiguous().float(), ray_d.reshape(-1, 3).contiguous().float(), float(np.float32(float(t)))

    def _ray_buffers(self, R, dev, t, flags, maps=True):
        """-> desc, workspace, (rgb, depth, acc, weights, counters) of a render of R rays at time t: the workspace as
        nvfi_render_workspace_bytes_t plans it, the outputs un-initialised (maps=False: no rgb / depth / acc - the caller has its own)"""
        desc = self._desc()
        nbytes = _lib.bytes_of(_lib.lib().nvfi_render_workspace_bytes_t, C.byref(desc), R, flags, t)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rgb, depth, acc = (torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)) if maps else (None, None, None)
        weights = torch.empty(R, desc.n_samples, device=dev)
        counters = torch.empty(_lib.NCOUNTERS, dtype=torch.int64, device=dev)
        return desc, ws, (rgb, depth, acc, weights, counters)

    def _ray_call(self, ray_o, ray_d, t, flags):
        """The set-up of a ray call: (ray_o, ray_d, t, flags) -> prepared rays and time, desc, workspace, the five standard outputs.  A caller
        that draws its jitter between the two halves (forward, render_mse_backward_) calls them itself."""
        ray_o, ray_d, t = self._prep_rays(ray_o, ray_d, t)
        return (ray_o, ray_d, t) + self._ray_buffers(ray_o.shape[0], ray_o.device, t, flags)

    def forward(self, t, ray_o, ray_d, white_bg=True, ndc_ray=False, N_samples=-1, transfer_vel=False):
        """render one chunk of rays (tensorf_keyframe.py:613-755) -> rgb, depth, acc, weights, mask_map."""
        if ndc_ray:
            raise NotImplementedError("ndc rays are out of scope (ndc: False in every shipped config)")
        if N_samples > 0 and N_samples != self.nSamples:
            raise NotImplementedError("per-call N_samples override is not supported")
        t_dev = getattr(t, "dev", None)
        ray_o, ray_d, t = self._prep_rays(ray_o, ray_d, t)
        R = ray_o.shape[0]
        training = self.training
        flags = 0
        jitter = None
        if training:
            flags |= _lib.NVFI_TRAIN
            if self.fork_backward:
                flags |= _lib.NVFI_BWD_FORK
            # the reference draws the per-ray jitter on the CPU generator (tensorf_base.py:302-306)
            jitter = self._jitter(R, ray_o.device)
        # white background or the training-time random-white coin, drawn on CPU (tensorf_keyframe.py:740)
        if white_bg or (training and bool(torch.rand((1,)) < 0.5)):
            flags |= _lib.NVFI_WHITE_BG
        if transfer_vel:
            flags |= _lib.NVFI_TRANSFER
        if self.mask_field is not None:
            flags |= _lib.NVFI_WANT_MASK
        if t_dev is not None:
            if self.mask_field is not None:
                raise NotImplementedError("DeviceTime renders do not support the mask branch")
            t = DeviceTime(t, t_dev)
        params = self._render_params()
        if training and self._use_side_streams():
            # the render runs on one of the field's two render streams (ordered behind everything queued on the caller's stream so far,
            # e.g. the last optimiser step); the caller's stream waits for the outputs.  Autograd runs the backward on this stream too.
            cur = torch.cuda.current_stream()
            side = self._side_stream("r")
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                rgb, depth, acc, weights, cnt = _RenderFn.apply(self, t, ray_o, ray_d, jitter, flags, *params)
            cur.wait_stream(side)
            for x in (rgb, depth, acc, weights, cnt):
                x.record_stream(cur)
            for x in (ray_o, ray_d, jitter):
                if x is not None:
                    x.record_stream(side)
        elif training and torch.is_grad_enabled():
            rgb, depth, acc, weights, _ = _RenderFn.apply(self, t, ray_o, ray_d, jitter, flags, *params)
        else:
            with torch.no_grad():
                rgb, depth, acc, weights, _ = _RenderFn.apply(self, t, ray_o, ray_d, jitter, flags, *params)
        if self.mask_field is None:
            # (R, 3) zeros like the reference's placeholder (tensorf_keyframe.py:673-676 without a mask_field) - a stride-0 view of one cached
            # zero instead of a fill launch per render; nobody writes into it
            z = _rt(self).get("_zero1")
            if z is None or z.device != ray_o.device:
                z = _rt(self)["_zero1"] = torch.zeros(1, 1, device=ray_o.device)
            mask_map = z.expand(R, 3)
        elif training and torch.is_grad_enabled():
            mask_map = self._mask_map_train(R, weights)
        else:
            mask_map = self._mask_map(t, flags, R, weights)
        return rgb, depth, acc, weights, mask_map

    @torch.no_grad()
    def render_flow(self, t, ray_o, ray_d, dt, camera=None, white_bg=True, transfer_vel=False):
        """Eval-mode render of one chunk of rays with the velocity field's maps (include/nvfi_hip.h: nvfi_render_flow; the reference has no
        counterpart) -> rgb, depth, acc, weights, vel_map (R,3), flow_map (R,3), flow2d (R,2) or None.

        Over the appearance-masked samples of a ray (weight > rayMarch_weight_thres, un-warped positions x_j at time t): vel_map = sum_j w_j *
        aabbSize/2 * v(x_j, t) in world units per unit time; flow_map = sum_j w_j * aabbSize/2 * (integrate_pos(x_j, t, t + dt) - x_j), the 3-D
        displacement over dt (dt > 0: forward in time; dt == 0: zeros); flow2d = the same displacement projected by `camera` (anything with
        pose / height / width / focal as models.Camera has them, or a tuple (pose3x4, H, W, focal)) in pixels, None without a camera.
        One nvfi_render_fwd plus one nvfi_render_flow on the same workspace: the masked count never reaches the host."""
        if self.training:
            raise NotImplementedError("render_flow is an inference branch: call .eval() first")
        if not self.use_vel:
            raise NotImplementedError("render_flow needs a velocity field (use_vel=False)")
        from ..utils.flow_loss import flow_camera
        L = _lib.lib()
        flags = _lib.NVFI_WANT_FLOW | (_lib.NVFI_WHITE_BG if white_bg else 0) | (_lib.NVFI_TRANSFER if transfer_vel else 0)
        ray_o, ray_d, t, desc, ws, (rgb, depth, acc, weights, counters) = self._ray_call(ray_o, ray_d, t, flags)
        R, dev = ray_o.shape[0], ray_o.device
        dt = float(np.float32(float(dt)))
        pose, H, W, focal = (None, 0, 0, 0.0) if camera is None else flow_camera(camera, dev)
        vel_map, flow_map = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
        flow2d = torch.zeros(R, 2, device=dev) if pose is not None else None
        if R > 0:
            _lib.check(L.nvfi_render_fwd(C.byref(desc), R, _lib.ptr(ray_o), _lib.ptr(ray_d), None, t, flags, _lib.ptr(rgb), _lib.ptr(depth),
                                         _lib.ptr(acc), _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.ptr(counters), _stream_ptr()))
            _lib.check(L.nvfi_render_flow(C.byref(desc), R, _lib.ptr(ray_o), _lib.ptr(ray_d), t, dt, flags, _lib.ptr(weights), _lib.ptr(pose),
                                          H, W, focal, _lib.ptr(vel_map), _lib.ptr(flow_map), _lib.ptr(flow2d), _lib.ptr(ws), ws.numel(),
                                          _stream_ptr()))
            self.last_counters = counters
        return rgb, depth, acc, weights, vel_map, flow_map, flow2d

    def _select_vector(self, select, dev):
        """`select` of render_objects as a float32 device tensor (K,) in [0, 1], or None.  Floating-point (or bool) entries: one factor per
        object, length K.  Integer entries: the indices of the objects to keep (everything else is removed)."""
        if select is None:
            return None
        K = self.mask_field.mask_dim
        if torch.is_tensor(select) and select.is_cuda and select.dtype == torch.float32 and select.numel() == K:
            return select.reshape(-1).to(dev).contiguous()      # already prepared (Renderer.render_objects): no host round trip per chunk
        sel = (select.detach().cpu() if torch.is_tensor(select) else torch.as_tensor(np.asarray(select)))
        if sel.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            idx = sel.reshape(-1).long()
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= K):
                raise ValueError(f"select: object index outside [0, {K})")
            out = torch.zeros(K, dtype=torch.float32)
            out[idx] = 1.0
            sel = out
        sel = sel.reshape(-1).to(torch.float32)
        if sel.numel() != K:
            raise ValueError(f"select: {sel.numel()} factors for a mask field of {K} objects")
        if bool((sel < 0).any()) or bool((sel > 1).any()):
            raise ValueError("select: factors must lie in [0, 1]")
        return sel.to(dev).contiguous()

    @torch.no_grad()
    def render_objects(self, t, ray_o, ray_d, select=None, white_bg=True, transfer_vel=False):
        """Eval-mode render of one chunk of rays with the per-object layers of the attached mask_field (include/nvfi_hip.h: nvfi_render_objects,
        nvfi_render_fwd_select; the reference has no counterpart) -> rgb, depth, acc, weights, mask_map (R,K), obj_rgb (R,K,3), obj_acc (R,K),
        obj_depth (R,K).

        Over the appearance-masked samples of a ray, with m_jk the MaskField softmax at the sample's warped keyframe position: obj_acc = sum_j w_j
        m_jk (= mask_map), obj_rgb = sum_j w_j m_jk c_j (premultiplied: no background, no clamp; summed over k it is the ray's colour before
        background and clamp), obj_depth = sum_j w_j m_jk z_j.  `select` (None: the plain render) re-renders the scene with objects removed, kept or
        faded: a length-K sequence / tensor of factors in [0, 1], or a list of INTEGER object indices to keep.  The density of every sample is
        scaled by sum_k select_k m_k(x) BEFORE the weights, so occlusion is recomputed: removing the object in front reveals what is behind it
        (utils.objects_vis.composite_layers, the 2-D recombination of finished layers, cannot).  The layers are then those of the selected render."""
        if self.training:
            raise NotImplementedError("render_objects is an inference branch: call .eval() first")
        if self.mask_field is None:
            raise NotImplementedError("render_objects needs a mask_field attached to the field")
        L = _lib.lib()
        mf = self.mask_field
        K = mf.mask_dim
        flags = _lib.NVFI_WANT_MASK | (_lib.NVFI_WHITE_BG if white_bg else 0) | (_lib.NVFI_TRANSFER if transfer_vel else 0)
        if select is not None:
            flags |= _lib.NVFI_WANT_SELECT
        ray_o, ray_d, t, desc, ws, (rgb, depth, acc, weights, counters) = self._ray_call(ray_o, ray_d, t, flags)
        R, dev = ray_o.shape[0], ray_o.device
        sel = self._select_vector(select, dev)
        md = _mask_desc(mf, mf._params())
        mask_map, obj_rgb = torch.zeros(R, K, device=dev), torch.zeros(R, K, 3, device=dev)
        obj_acc, obj_depth = torch.zeros(R, K, device=dev), torch.zeros(R, K, device=dev)
        if R > 0:
            _lib.check(L.nvfi_render_fwd_select(C.byref(desc), C.byref(md), _lib.ptr(sel), R, _lib.ptr(ray_o), _lib.ptr(ray_d), None, t, flags,
                                                _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(weights), _lib.ptr(ws), ws.numel(),
                                                _lib.ptr(counters), _stream_ptr()))
            _lib.check(L.nvfi_render_mask(C.byref(desc), C.byref(md), R, t, flags, _lib.ptr(weights), _lib.ptr(mask_map), _lib.ptr(ws),
                                          ws.numel(), _stream_ptr()))
            _lib.check(L.nvfi_render_objects(C.byref(desc), C.byref(md), R, t, flags, _lib.ptr(weights), _lib.ptr(obj_rgb), _lib.ptr(obj_acc),
                                             _lib.ptr(obj_depth), _lib.ptr(ws), ws.numel(), _stream_ptr()))
            self.last_counters = counters
        return rgb, depth, acc, weights, mask_map, obj_rgb, obj_acc, obj_depth

    def _mask_map_train(self, R, weights):
        """Train-mode mask branch (tensorf_keyframe.py:673-676, 749-753), differentiable like the reference's: the appearance-masked
        samples of the render call are exported (warped keyframe positions), MaskField runs through its own autograd boundary
        (nvfi_maskfield_fwd / _bwd), and the composite sum_j w_j mask_j is a torch index_add - so gradients reach the MaskField
        parameters and, through `weights`, the density branch of the field.  (The points themselves carry no gradient: MaskField's
        kernels do not differentiate their input, as in train_segm.py where they are computed under no_grad.  No reference script
        differentiates this branch: test_segm_render.py:96 renders in test mode.)"""
        L = _lib.lib()
        R_, t, flags = self._last_call
        desc = self._desc()
        M = int(self.last_counters[2])          # host value: sizes the export (the reference syncs here too: `if app_mask.any()`)
        K = self.mask_field.mask_dim
        dev = weights.device
        if M == 0:
            return weights.sum(-1, keepdim=True) * torch.zeros(1, K, device=dev)
        xyz = torch.empty(M, 3, device=dev)
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        ws = self._last_ws
        _lib.check(L.nvfi_render_export_masked(C.byref(desc), R, t, flags, _lib.ptr(ws), ws.numel(), M, _lib.ptr(xyz), _lib.ptr(idx), _stream_ptr()))
        mask = self.mask_field(xyz)
        S = weights.shape[1]
        w = weights.reshape(-1)[idx]
        return torch.zeros(R, K, device=dev).index_add(0, idx // S, w[:, None] * mask)

    @torch.no_grad()
    def _mask_map(self, t, flags, R, weights):
        """mask branch of render_pts (tensorf_keyframe.py:673-676, 749-753); inference only."""
        L = _lib.lib()
        mf = self.mask_field
        md = _mask_desc(mf, mf._params())
        out = torch.empty(R, mf.mask_dim, device=weights.device)
        desc = self._desc()
        ws = self._last_ws
        _lib.check(L.nvfi_render_mask(C.byref(desc), C.byref(md), R, t, flags, _lib.ptr(weights.detach()), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                      _stream_ptr()))
        return out

    # ------------------------------------------------------------------ building blocks (inference, no autograd)
    def normalize_coord(self, xyz_sampled):
        return (xyz_sampled - self.aabb[0]) * self.invaabbSize - 1

    def normalize_time_coord(self, time):
        if self.num_keyframes == 1 or self.tmax == 0:
            return time * 0
        return time * 2 / self.tmax - 1

    @torch.no_grad()
    def _vel_eval(self, xt, gated):
        if not self.use_vel:
            raise _lib.NvfiError("vel / vel_net needs a field with a velocity net (use_vel)")
        L = _lib.lib()
        xt = xt.reshape(-1, 4).contiguous().float()
        N = xt.shape[0]
        desc = self._desc()
        nb = _lib.bytes_of(L.nvfi_vel_workspace_bytes, C.byref(desc), N)
        ws = torch.empty(nb, dtype=torch.uint8, device=xt.device)
        u = torch.zeros(N, 6, device=xt.device)
        _lib.check(L.nvfi_vel_eval(C.byref(desc), N, _lib.ptr(xt), _lib.ptr(u), int(gated), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        return u[:, :3].contiguous() if gated else u

    @torch.no_grad()
    def integrate_pos(self, pos_init, t, base_times):
        """RK2 back-advection with per-point times (tensorf_keyframe.py:575-611). Unlike the reference this
        does not mutate its arguments."""
        if not self.use_vel:
            raise _lib.NvfiError("integrate_pos needs a field with a velocity net (use_vel)")
        L = _lib.lib()
        x = pos_init.reshape(-1, 3).contiguous().float()
        tt = t.reshape(-1).contiguous().float()
        bb = base_times.reshape(-1).contiguous().float()
        N = x.shape[0]
        desc = self._desc()
        nb = _lib.bytes_of(L.nvfi_vel_workspace_bytes, C.byref(desc), N)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        out = torch.empty_like(x)
        _lib.check(L.nvfi_integrate_pos(C.byref(desc), N, _lib.ptr(x), _lib.ptr(tt), _lib.ptr(bb), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _stream_ptr()))
        return out

    def advect(self, pos, t, t_target, max_workspace_bytes=1 << 30):
        """integrate_pos(pos, t, t_target) for scalar times WITH gradients (tensorf_keyframe.py:575-611 under autograd): a loss on the advected
        points reaches `pos` and the 12 tensors of vel_net.weight_net - 3-D track / scene-flow / optical-flow supervision, cycle consistency,
        trajectory smoothness.  Every gate / rejection decision is held fixed; a_weight_net and the planes get nothing; no second-order gradients.
        The value is integrate_pos' bit for bit.  The backward recomputes the warp in chunks whose workspace stays under `max_workspace_bytes`.
        Under no_grad, or when neither `pos` nor a weight_net parameter requires grad, this is exactly integrate_pos (tensor times allowed).
        More than 64 RK2 steps between the two scalar times is refused (error 2), not truncated."""
        if not (isinstance(pos, torch.Tensor) and pos.is_cuda):
            raise _lib.NvfiError("advect needs its points on the GPU (no CPU fallback exists)")
        if not self.use_vel:
            raise _lib.NvfiError("advect needs a field with a velocity net (use_vel)")
        wparams = self._render_params()[fs.WEIGHT_NET]
        wants = torch.is_grad_enabled() and (pos.requires_grad or any(p.requires_grad for p in wparams))

        def scalar(v):
            if isinstance(v, torch.Tensor):
                if v.numel() == 0 or bool((v != v.reshape(-1)[0]).any()):
                    return None
                v = v.reshape(-1)[0].item()
            return float(np.float32(float(v)))

        ts, t1s = scalar(t), scalar(t_target)
        if ts is None or t1s is None:
            if wants:
                raise NotImplementedError("advect: per-point times (a tensor t / t_target with more than one distinct value) have no gradient path "
                                          "here: use advect_pt")
            return self.integrate_pos(pos, t, t_target).reshape(pos.shape)
        desc = self._desc()
        if wants and (desc.vel_fp16 & 3) in (1, 2):
            raise NotImplementedError("advect: the fp16-input modes (vel_fp16 1 / 2) have no adjoint")
        if (desc.vel_fp16 & 3) not in (1, 2):      # the step limit, decided on the host before anything is launched
            _lib.bytes_of(_lib.lib().nvfi_advect_grad_workspace_bytes, C.byref(desc), 0, ts, t1s)
        x = pos.reshape(-1, 3).contiguous().float()
        if not wants:
            tt = torch.full((x.shape[0],), ts, dtype=torch.float32, device=x.device)
            return self.integrate_pos(x, tt, torch.full_like(tt, t1s)).reshape(pos.shape)
        return _AdvectFn.apply(self, x, ts, t1s, int(max_workspace_bytes), *wparams).reshape(pos.shape)

    def advect_pt(self, pos, t, t_target, max_workspace_bytes=1 << 30):
        """`advect` with PER-POINT times: integrate_pos(pos_i, t_i, t_target_i) WITH gradients to `pos` and the 12 tensors of vel_net.weight_net,
        for tracks that start at many frame times, random time pairs, points of all frames warped to their own keyframe - one call instead of
        one `advect` per distinct pair.  `t` and `t_target` are each a Python float or a device tensor of N / (N,1) elements.  The times carry
        NO gradient: a time tensor that requires grad is refused.  Every rule of `advect` holds (decisions held fixed, no second-order gradients,
        the value is integrate_pos' bit for bit, vel_fp16 modes 1 / 2 have no adjoint).  A point more than 64 RK2 steps from its target is
        refused (NvfiError, error 2) before anything is launched, not truncated.
        ONE HOST SYNCHRONISATION per call with gradients: the forward reads the 66-bin histogram of the points' step counts (so the call cannot
        be captured in a hipGraph).  The backward sorts the points by step count and runs every step count as chunks of its own, each under
        `max_workspace_bytes`, so its cost follows the sum of the steps; zero-step points launch nothing.  `last_advect_pt_chunks` is the list of
        (points, max_steps) it ran, `last_advect_pt_workspace_bytes` the workspace it took; the gradient comes back in the caller's order.
        Under no_grad, or when neither `pos` nor a weight_net parameter requires grad, this is exactly integrate_pos."""
        for name, v in (("t", t), ("t_target", t_target)):
            if isinstance(v, torch.Tensor) and v.requires_grad:
                raise _lib.NvfiError(f"advect_pt: {name} requires grad, but the times get no gradient (detach it)")
        if not (isinstance(pos, torch.Tensor) and pos.is_cuda):
            raise _lib.NvfiError("advect_pt needs its points on the GPU (no CPU fallback exists)")
        if not self.use_vel:
            raise _lib.NvfiError("advect_pt needs a field with a velocity net (use_vel)")
        x = pos.reshape(-1, 3).contiguous().float()
        N = x.shape[0]

        def times(v, name):
            if isinstance(v, torch.Tensor):
                if not v.is_cuda:
                    raise _lib.NvfiError(f"advect_pt needs {name} on the GPU (no CPU fallback exists)")
                if v.numel() != N:
                    raise _lib.NvfiError(f"advect_pt: {name} has {v.numel()} elements for {N} points")
                return v.detach().reshape(-1).contiguous().float()
            return torch.full((N,), float(v), dtype=torch.float32, device=x.device)

        tt, t1 = times(t, "t"), times(t_target, "t_target")
        wparams = self._render_params()[fs.WEIGHT_NET]
        wants = torch.is_grad_enabled() and (pos.requires_grad or any(p.requires_grad for p in wparams))
        if not wants:
            return self.integrate_pos(x, tt, t1).reshape(pos.shape)
        if (self._desc().vel_fp16 & 3) in (1, 2):
            raise NotImplementedError("advect_pt: the fp16-input modes (vel_fp16 1 / 2) have no adjoint")
        return _AdvectPtFn.apply(self, x, tt, t1, int(max_workspace_bytes), *wparams).reshape(pos.shape)

    @torch.no_grad()
    def compute_densityfeature(self, xyzt):
        """(N,4) normalised (x,y,z,t') -> (N,1) (tensorf_keyframe.py:233-272)."""
        L = _lib.lib()
        q = xyzt.reshape(-1, 4).contiguous().float()
        N = q.shape[0]
        feat = torch.empty(N, device=q.device)
        sigma = torch.empty(N, device=q.device)
        desc = self._desc()
        _lib.check(L.nvfi_density_at(C.byref(desc), N, _lib.ptr(q), _lib.ptr(feat), _lib.ptr(sigma), _stream_ptr()))
        return feat.unsqueeze(-1)

    def lookup_density(self, xyzt):
        """compute_densityfeature WITH gradients (tensorf_keyframe.py:233-272 under autograd): (N,4) normalised (x,y,z,t') -> (N,1), differentiable
        once to `xyzt` (all four columns) and to the six density planes - Lagrangian losses on advected points (`advect`), free-space / occupancy
        losses from depth sensors, sparsity on random points, distillation.  sigma follows through feature2density (a torch softplus).  The value
        is compute_densityfeature's bit for bit; under no_grad, or when neither `xyzt` nor a density plane requires grad, this IS that call.
        The plane gradients are float atomics (not bit-repeatable); the gradient at `xyzt` repeats bit for bit."""
        if not (isinstance(xyzt, torch.Tensor) and xyzt.is_cuda):
            raise _lib.NvfiError("lookup_density needs its points on the GPU (no CPU fallback exists)")
        planes = self._render_params()[fs.DENSITY]
        if not (torch.is_grad_enabled() and (xyzt.requires_grad or any(p.requires_grad for p in planes))):
            return self.compute_densityfeature(xyzt)
        return _DensityLookupFn.apply(self, xyzt.reshape(-1, 4).contiguous().float(), *planes)

    def lookup_appfeature(self, xyzt):
        """compute_appfeature WITH gradients (tensorf_keyframe.py:274-310 under autograd): (N,4) -> (N, app_dim), differentiable once to `xyzt`, the
        six appearance planes and basis_mat.weight.  renderModule on these features stays forward-only."""
        if not (isinstance(xyzt, torch.Tensor) and xyzt.is_cuda):
            raise _lib.NvfiError("lookup_appfeature needs its points on the GPU (no CPU fallback exists)")
        params = self._render_params()[fs.APP]
        if not (torch.is_grad_enabled() and (xyzt.requires_grad or any(p.requires_grad for p in params))):
            return self.compute_appfeature(xyzt)
        return _AppLookupFn.apply(self, xyzt.reshape(-1, 4).contiguous().float(), *params)

    @torch.no_grad()
    def compute_appfeature(self, xyzt):
        """(N,4) normalised (x,y,z,t') -> (N, app_dim) (tensorf_keyframe.py:274-310); forward only, like compute_densityfeature."""
        from ..utils import field_lookup as fl
        if not (isinstance(xyzt, torch.Tensor) and xyzt.is_cuda):
            raise _lib.NvfiError("compute_appfeature needs its points on the GPU (no CPU fallback exists)")
        return fl.appfeat_raw(self._desc(), xyzt)

    @staticmethod
    @torch.no_grad()
    def sh_render(viewdirs, features):
        """SHRender (tensorf_model_utils.py:292-296): degree-2 real SH, relu(sum + 0.5); features (N,27)."""
        L = _lib.lib()
        v = viewdirs.reshape(-1, 3).contiguous().float()
        ft = features.reshape(-1, 27).contiguous().float()
        rgb = torch.empty(v.shape[0], 3, device=v.device)
        _lib.check(L.nvfi_sh_render(v.shape[0], _lib.ptr(v), _lib.ptr(ft), _lib.ptr(rgb), _stream_ptr()))
        return rgb

    def feature2density(self, density_features, x=None):
        return F.softplus(density_features[..., 0] + self.density_shift)

    @torch.no_grad()
    def app_at(self, xyzt, viewdirs):
        """compute_appfeature + renderModule for explicit points (tensorf_keyframe.py:274-310, tensorf_base.py:88-98)."""
        L = _lib.lib()
        q = xyzt.reshape(-1, 4).contiguous().float()
        v = viewdirs.reshape(-1, 3).contiguous().float()
        N = q.shape[0]
        rgb = torch.empty(N, 3, device=q.device)
        desc = self._desc()
        nb = _lib.bytes_of(L.nvfi_app_workspace_bytes, C.byref(desc), N)
        ws = torch.empty(nb, dtype=torch.uint8, device=q.device)
        _lib.check(L.nvfi_app_at(C.byref(desc), N, _lib.ptr(q), _lib.ptr(v), _lib.ptr(rgb), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        return rgb

    def _render_module_call(self, pts, viewdirs, features):
        L = _lib.lib()
        if not features.is_cuda:
            raise _lib.NvfiError("NVFi HIP kernels need CUDA tensors (no CPU fallback exists)")
        x = pts.reshape(-1, 3).contiguous().float()
        v = viewdirs.reshape(-1, 3).contiguous().float()
        fe = features.reshape(-1, self.app_dim).contiguous().float()
        N = x.shape[0]
        rgb = torch.empty(N, 3, device=x.device)
        desc = self._desc()
        nb = _lib.bytes_of(L.nvfi_app_workspace_bytes, C.byref(desc), N)
        ws = torch.empty(2 * nb, dtype=torch.uint8, device=x.device)
        _lib.check(L.nvfi_render_mlp(C.byref(desc), N, _lib.ptr(x), _lib.ptr(v), _lib.ptr(fe), _lib.ptr(rgb), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        return rgb

    def shade(self, pts, viewdirs, features, max_workspace_bytes=1 << 30):
        """renderModule(pts, viewdirs, features) WITH gradients (tensorf_base.py:88-98, or SHRender, under autograd): (N,3), (N,3), (N, app_dim) ->
        (N,3), differentiable once to `features`, `pts`, `viewdirs` and the six tensors of renderModule.mlp - colour constancy along a trajectory
        (`advect`), colour supervision from RGB-D point clouds, distillation of radiance, pose / direction refinement.  The value is
        renderModule's bit for bit; under no_grad, or when nothing requires grad, this IS _render_module_call.  The backward runs the forward again
        in chunks whose workspace stays under `max_workspace_bytes` (nvfi_render_mlp_grad).  Per-point gradients repeat bit for bit."""
        if not all(isinstance(a, torch.Tensor) and a.is_cuda for a in (pts, viewdirs, features)):
            raise _lib.NvfiError("shade needs its points, view directions and features on the GPU (no CPU fallback exists)")
        mlp = [p for p in self._render_params()[fs.RENDER_MLP] if p is not None]
        if not (torch.is_grad_enabled() and any(a.requires_grad for a in [pts, viewdirs, features] + mlp)):
            return self._render_module_call(pts, viewdirs, features)
        return _ShadeFn.apply(self, pts.reshape(-1, 3).contiguous().float(), viewdirs.reshape(-1, 3).contiguous().float(),
                              features.reshape(-1, self.app_dim).contiguous().float(), int(max_workspace_bytes), *mlp)

    def lookup_rgb(self, xyzt, viewdirs, max_workspace_bytes=1 << 30):
        """shade(xyzt[:, :3], viewdirs, lookup_appfeature(xyzt)): the colour of given points (N,4) normalised (x,y,z,t') with gradients to the points
        (t' included), the six appearance planes, basis_mat.weight and the MLP.  The value is renderModule(xyz, view, compute_appfeature(xyzt))
        bit for bit; it agrees with app_at only to rounding (app_at forms the features on the MFMA path inside its kernel)."""
        if not (isinstance(xyzt, torch.Tensor) and xyzt.is_cuda):
            raise _lib.NvfiError("lookup_rgb needs its points on the GPU (no CPU fallback exists)")
        q = xyzt.reshape(-1, 4)
        return self.shade(q[:, :3], viewdirs, self.lookup_appfeature(q), max_workspace_bytes=max_workspace_bytes)

    def pde_loss(self, points, t):
        """PDE regulariser on explicit collocation points (world-space (P,3), raw t (P,1)); models/nvfi.py:42-84."""
        points = points.reshape(-1, 3).contiguous().float()
        t = t.reshape(-1).contiguous().float()
        if self._use_side_streams():
            cur = torch.cuda.current_stream()
            side = self._side_stream("p")
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                loss = _PdeFn.apply(self, points, t, *self._pde_params())
            cur.wait_stream(side)
            loss.record_stream(cur)
            points.record_stream(side); t.record_stream(side)
            return loss
        return _PdeFn.apply(self, points, t, *self._pde_params())

    @torch.no_grad()
    def pde_loss_backward_(self, points, t, weight=1.0, grad_targets=None):
        """Fused value + backward of `weight * get_vel_loss`: the gradient is ACCUMULATED into the .grad of both velocity
        nets (or into `grad_targets`, 24 tensors in _pde_params() order); returns the device tensor
        [loss, n_kept, sum div^2, sum transport^2] (un-weighted loss)."""
        L = _lib.lib()
        points = points.reshape(-1, 3).contiguous().float()
        t = t.reshape(-1).contiguous().float()
        P = points.shape[0]
        desc = self._desc()
        nbytes = _lib.bytes_of(L.nvfi_pde_workspace_bytes, C.byref(desc), P)
        ws = self._scratch("pde", nbytes, points.device)
        out = torch.empty(4, device=points.device)       # written by k_pde_finish
        if grad_targets is not None:
            grads = list(grad_targets)
        else:
            grads, _ = self._grad_targets(self._pde_params(), [True] * fs.N_PDE, mode=True)
        G = self._grads_struct_vel(grads)
        counters = torch.empty(_lib.NCOUNTERS, dtype=torch.int64, device=points.device)
        # no host_info: the call does not wait for the device; the kept count is out[1] / counters[4] (device side)
        if isinstance(weight, torch.Tensor):     # the weight lives in device memory (hipGraph replay: it decays every iteration)
            if not (weight.is_cuda and weight.dtype == torch.float32 and weight.numel() == 1):
                raise _lib.NvfiError("a device-side PDE weight must be a 1-element fp32 CUDA tensor")
            _lib.check(L.nvfi_pde_loss_dev(C.byref(desc), P, _lib.ptr(points), _lib.ptr(t), _lib.ptr(weight), _lib.ptr(out), C.byref(G), _lib.ptr(ws),
                                           ws.numel(), _lib.ptr(counters), _stream_ptr()))
        else:
            _lib.check(L.nvfi_pde_loss_ex(C.byref(desc), P, _lib.ptr(points), _lib.ptr(t), float(weight), _lib.ptr(out), C.byref(G), _lib.ptr(ws),
                                          ws.numel(), _lib.ptr(counters), None, None, 0, None, _stream_ptr()))
        self.last_pde_out, self.last_pde_counters = out, counters
        self.last_pde_n_kept = None
        return out

    # ------------------------------------------------------------------ characteristic loss (csrc/charloss.hip)
    def characteristic_time(self, t):
        """the keyframe time t_k the characteristic loss runs at (tensorf_keyframe.py:554-561, fp32): the nearest keyframe time for t > 0,
        the first keyframe interval tmax / (K - 1) otherwise.  Host arithmetic; nvfi_char_loss derives the same number."""
        K = int(self.num_keyframes)
        t = np.float32(float(t))
        if t > 0:
            ts = np.float32(float(self.tmax) / (K - 1) if K > 1 else 1.0)
            return float(np.rint(np.clip(t / ts, np.float32(0), np.float32(K - 1))) * ts)
        return float(np.float32(float(self.tmax)) / np.float32(K - 1))

    def _char_call(self, points, t, weight, grads, params=None):
        """one nvfi_char_loss launch sequence -> (terms (2,), points0 (N,3)); grads: 13 tensors or None entries (dps, dpt, aps, apt, basis_mat)"""
        if not self.use_vel:
            raise _lib.NvfiError("characteristic_loss needs the velocity field (use_vel=False): there is nothing to advect the points with")
        if not (self.aabb.is_cuda and points.is_cuda):
            raise _lib.NvfiError("NVFi HIP kernels need the field and the points on the GPU (no CPU fallback exists)")
        L = _lib.lib()
        pts = points.detach().reshape(-1, 3).contiguous().float()
        N = pts.shape[0]
        desc = self._desc() if params is None else self._desc(self._params_with(fs.PLANES, params))
        nb = _lib.bytes_of(L.nvfi_char_workspace_bytes, C.byref(desc), N)
        ws = self._scratch("char", nb, pts.device)
        terms = torch.empty(2, device=pts.device)
        points0 = torch.empty_like(pts)
        G = None
        if grads is not None:
            for g, p in zip(grads, self._render_params()[fs.PLANES]):
                if g is not None and g.stride() != p.stride():
                    raise _lib.NvfiError("a gradient target must share the memory layout of its parameter (channels_last planes)")
            G = C.byref(self._grads_struct(list(grads)))
        _lib.check(L.nvfi_char_loss(C.byref(desc), N, _lib.ptr(pts), float(t), float(weight), _lib.ptr(terms), _lib.ptr(points0), G, _lib.ptr(ws),
                                    ws.numel(), _stream_ptr()))
        return terms, points0

    def characteristic_loss_at(self, points, t, return_points0=False):
        """characteristic_loss for caller-supplied normalised points (N,3): mean (d_t - d_0)^2 + mean (a_t - a_0)^2 between keyframe
        t_k = characteristic_time(t) at `points` and keyframe 0 at points0 = integrate_pos(points, t_k, 0) (no gradient through the warp).  A 0-dim
        tensor with autograd history onto the twelve planes and basis_mat; the two terms of the last call are kept in `last_char_terms`."""
        if not self.use_vel:
            raise _lib.NvfiError("characteristic_loss needs the velocity field (use_vel=False): there is nothing to advect the points with")
        loss, terms, points0 = _CharFn.apply(self, points, float(t), *self._render_params()[fs.PLANES])
        self.last_char_terms = terms
        return (loss, points0) if return_points0 else loss

    def characteristic_loss(self, n_pts, t):
        """tensorf_keyframe.py:552-573 with the semantics of its formula (t_k and the points as they were before the warp; the reference's own
        call aliases both): n_pts points uniform in [-1,1]^3, drawn with torch.rand on the field's device."""
        if not self.aabb.is_cuda:
            raise _lib.NvfiError("NVFi HIP kernels need the field on the GPU (no CPU fallback exists)")
        points = torch.rand(int(n_pts), 3, device=self.aabb.device) * 2 - 1
        return self.characteristic_loss_at(points, t)

    @torch.no_grad()
    def characteristic_loss_backward_(self, points_or_n, t, weight=1.0):
        """Fused value + backward of `weight * characteristic_loss`: the gradient is ACCUMULATED into the .grad of the twelve planes and
        basis_mat (a tensor with requires_grad=False is left alone); returns the detached UN-weighted value (0-dim; `last_char_terms` holds
        the density and the appearance term).  points_or_n: normalised points (N,3) or a point count (drawn as characteristic_loss does)."""
        if not self.aabb.is_cuda:
            raise _lib.NvfiError("NVFi HIP kernels need the field on the GPU (no CPU fallback exists)")
        if isinstance(points_or_n, torch.Tensor):
            points = points_or_n
        else:
            points = torch.rand(int(points_or_n), 3, device=self.aabb.device) * 2 - 1
        params = self._render_params()[fs.PLANES]
        grads, _ = self._grad_targets(params, [p.requires_grad for p in params], mode=True)
        terms, _ = self._char_call(points, t, weight, grads)
        self.last_char_terms = terms
        return terms[0] + terms[1]

    def _grads_struct_cached(self, ps):
        """nvfi_grads over the .grad tensors of the 31 render parameters (NULL for a parameter that is frozen or has no .grad): the ctypes
        struct is rebuilt only when a gradient pointer changed (a GradBucket / the arena keeps them fixed for the whole run)"""
        gs = [None if (p is None or p.grad is None or not p.requires_grad) else p.grad for p in ps]
        key = tuple(0 if g is None else g.data_ptr() for g in gs)
        c = _rt(self).get("_gs_cache")
        if c is None or c[0] != key:
            for g, p in zip(gs, ps):
                if g is not None and g.stride() != p.stride():
                    raise _lib.NvfiError("a parameter's .grad must share its memory layout (channels_last planes)")
            c = (key, self._grads_struct(gs))
            _rt(self)["_gs_cache"] = c
        return c[1]

    @torch.no_grad()
    def render_mse_backward_(self, t, ray_o, ray_d, target, white_bg=True, loss_scale=1.0, jitter=None, wait_before_backward=None,
                             target_depth=None, depth_index=None, depth_weight=1.0, skip_holes=False, check_depth_index=False,
                             distortion_weight=0.0, target_flow=None, flow_dt=None, flow_camera=None, flow_weight=1.0, flow_valid=None,
                             flow_kind="l2", flow_huber_delta=1.0, flow_max_workspace_bytes=1 << 30,
                             target_mask=None, mask_field=None, mask_weight=1.0, mask_kind="ce", mask_eps=1e-5, mask_max_workspace_bytes=1 << 30):
        """Fused-driver form of one TRAINING render of train_nvfi.py:150-178 + its share of loss.backward() (train_nvfi.py:242):
        forward, `loss_scale * F.mse_loss(rgb_map, target)` and the backward of both, with the parameter gradients ACCUMULATED into p.grad
        (which must exist: nvfi_amd.dist.GradBucket, or zeros_like) - no autograd graph, no torch launch: nvfi_render_fwd_mse forms the loss and
        its gradient inside the composite kernel, nvfi_render_bwd_t takes it from there.  The counterpart of pde_loss_backward_ /
        regularizers_backward_ for the photometric term.  Returns (loss, rgb): a 0-dim device tensor with the UN-scaled mse and the (R,3) colours.
        wait_before_backward: a stream the backward half has to wait for (a driver that runs regularizers_backward_ - a plain read-modify-write of
        the plane gradients - on a side stream beside the forward half).
        target_depth (default None: nothing changes, the same launches and the same two return values): depth supervision, the reference's
        `compute_depth_loss(depth_map, target_dpts)` (utils/evaluation_utils.py:8-17; Camera(..., dpt=) makes sample_rays return target_dpts).
        One nvfi_depth_loss launch between the two halves reads the depth map of the forward and writes
        `loss_scale * depth_weight * d(depth loss)/d(depth)`, which the backward half takes as its depth gradient - no torch launch.  Returns
        (loss, rgb, depth_loss), depth_loss the UN-scaled, un-weighted value (0-dim device tensor).  target_depth is (R,) fp32, or - with
        depth_index, the int64 pixel_ids of nvfi_draw_batch - a whole depth image read at depth_index[i] for ray i (no gather launch).  The
        kernel does not range-check the indices: they are the caller's contract, as pixel_ids drawn for an image of target_depth's size are.
        check_depth_index=True (a debugging aid: one torch min / max and a wait for it, before anything is launched) raises IndexError on an
        index outside the image.  skip_holes=True counts ray i only if its target depth is finite and > 0.  Multi-GPU: every rank
        normalises its OWN shard of the batch (its own medians); there is no global median.
        distortion_weight (default 0.0: nothing changes, the same launches and the same return values): the distortion loss of the ray
        weights (Mip-NeRF 360; utils.ray_regs.distortion_loss with delta = self.distortion_delta()).  With a positive weight one
        nvfi_ray_distortion call between the two halves reads the weights of the forward and writes
        `loss_scale * distortion_weight * d(distortion loss)/d(weights)` into a scratch (R, S), which the backward half takes as its weight
        gradient - no torch launch.  The UN-scaled, un-weighted value (0-dim device tensor) is appended as the LAST element of the returned
        tuple: (loss, rgb, distortion) or (loss, rgb, depth_loss, distortion).  Multi-GPU: every rank's mean is over its OWN shard of the batch.
        target_flow (default None: nothing changes, the same launches and the same return values): optical-flow supervision (flow_loss; the
        definition is in include/nvfi_hip.h).  (R, 2) target flow in pixels over flow_dt for the camera flow_camera, flow_valid an optional
        per-ray mask, flow_kind "l2" / "huber".  One nvfi_flow_loss_fwd between the two halves, behind the distortion call (it then ADDS its
        `loss_scale * flow_weight * d(flow loss)/d(weights)` to that call's scratch), and the chunked nvfi_flow_loss_bwd beside the backward
        half, into the same gradient buffers - no torch launch, PROVIDED the inputs arrive ready: target_flow a contiguous float32 (R, 2) device
        tensor, the pose of flow_camera a float32 device tensor and flow_valid a contiguous uint8 device tensor.  A host pose is copied to the
        device and a bool / float mask converted with a torch launch on every call (utils.flow_loss.flow_loss_raw); convert them once outside
        a loop or a captured graph.  The UN-scaled, un-weighted value (0-dim device tensor) is appended behind the distortion value.  The mask
        branch and DeviceTime renders raise NotImplementedError.
        target_mask (default None: nothing changes, the same launches, return values and refusals): 2-D mask supervision (mask_loss; the
        definition is in include/nvfi_hip.h) of the MaskField `mask_field` (default self.mask_field): int (R) labels or float (R, K) rows,
        mask_kind "ce" / "l2".  One nvfi_mask_loss_fwd between the two halves, behind the distortion and flow calls (it then ADDS its
        `loss_scale * mask_weight * d(mask loss)/d(weights)` to their scratch), and the chunked nvfi_mask_loss_bwd behind the backward half,
        ACCUMULATED into the .grad of the mask field's ten parameters, which must exist - no torch launch when target_mask arrives as
        contiguous int32 labels or contiguous float32 rows.  The UN-scaled, un-weighted value (0-dim device tensor) is appended LAST."""
        L = _lib.lib()
        t_dev = getattr(t, "dev", None)
        ray_o, ray_d, t = self._prep_rays(ray_o, ray_d, t)
        if self.mask_field is not None and target_mask is None:
            raise NotImplementedError("render_mse_backward_ does not drive the mask branch")
        if target_mask is not None:
            if t_dev is not None:
                raise NotImplementedError("render_mse_backward_: the mask term does not support DeviceTime renders")
            mask_field = self._mask_field_arg(mask_field, "render_mse_backward_(target_mask=)")
            mparams = mask_field._params()
            if any(p.requires_grad and (p.grad is None or not p.grad.is_contiguous()) for p in mparams):
                raise _lib.NvfiError("render_mse_backward_(target_mask=) accumulates into the .grad of the mask field's parameters: they must exist")
        distortion_weight = float(distortion_weight)
        if not distortion_weight >= 0.0:
            raise ValueError(f"distortion_weight must not be negative ({distortion_weight})")
        if target_flow is not None:
            if t_dev is not None:
                raise NotImplementedError("render_mse_backward_: the flow term does not support DeviceTime renders")
            if flow_dt is None or flow_camera is None:
                raise ValueError("target_flow needs flow_dt and flow_camera")
            if not self.use_vel:
                raise _lib.NvfiError("the flow term needs a field with a velocity net (use_vel)")
        target = target.reshape(-1, 3).contiguous().float()
        R = ray_o.shape[0]
        dev = ray_o.device
        flags = _lib.NVFI_TRAIN | (_lib.NVFI_BWD_FORK if self.fork_backward else 0)
        if jitter is None:
            jitter = self._jitter(R, dev)          # the reference's CPU-generator draw (tensorf_base.py:302-306)
        if white_bg or bool(torch.rand((1,)) < 0.5):    # tensorf_keyframe.py:740
            flags |= _lib.NVFI_WHITE_BG
        ps = self._render_params()
        desc, ws, (_, _, _, weights, counters) = self._ray_buffers(R, dev, t, flags, maps=False)
        S = desc.n_samples
        a3, a1 = round64(3 * R), round64(R)          # rgb | g_rgb | depth | acc | loss [| g_depth] [| distortion workspace]: one allocation, 256-byte aligned pieces
        o_gd = 2 * a3 + 2 * a1 + 64
        o_dw = o_gd + (a1 if target_depth is not None else 0)          # R doubles for nvfi_ray_distortion's mean: 2 * a1 floats
        out = torch.empty(o_dw + (2 * a1 if distortion_weight > 0.0 else 0), device=dev)
        rgb, g_rgb, depth, acc, loss = out[:3 * R].view(R, 3), out[a3:a3 + 3 * R], out[2 * a3:2 * a3 + R], out[2 * a3 + a1:2 * a3 + a1 + R], out[o_gd - 64:o_gd]
        g_depth = None
        if target_depth is not None:
            if not target_depth.is_cuda or (depth_index is not None and not depth_index.is_cuda):
                raise _lib.NvfiError("NVFi HIP kernels need the depth target on the GPU (no CPU fallback exists)")
            if target_depth.dtype != torch.float32 or not target_depth.is_contiguous():
                raise ValueError("target_depth must be a contiguous float32 tensor")
            if depth_index is not None:
                if depth_index.dtype != torch.int64 or not depth_index.is_contiguous() or depth_index.numel() != R:
                    raise ValueError(f"depth_index must be a contiguous int64 tensor with one entry per ray ({R})")
                if check_depth_index:
                    lo, hi = (int(v) for v in torch.aminmax(depth_index))
                    if lo < 0 or hi >= target_depth.numel():
                        raise IndexError(f"depth_index holds {lo if lo < 0 else hi}, outside the {target_depth.numel()} entries of target_depth")
            elif target_depth.numel() != R:
                raise ValueError(f"target_depth must hold one depth per ray ({R}) unless depth_index selects from an image")
            g_depth = out[o_gd:o_gd + R]
        st = _stream_ptr()
        _lib.check(L.nvfi_render_fwd_mse(C.byref(desc), R, _lib.ptr(ray_o), _lib.ptr(ray_d), _lib.ptr(jitter), t, _lib.ptr(t_dev), flags, _lib.ptr(rgb),
                                         _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.ptr(counters),
                                         _lib.ptr(target), float(loss_scale), _lib.ptr(loss), _lib.ptr(g_rgb), st))
        self.last_counters = counters
        if g_depth is not None:       # the int64 count of the entries that took part sits behind the depth loss
            _lib.check(L.nvfi_depth_loss(R, _lib.ptr(depth), _lib.ptr(target_depth), _lib.ptr(depth_index),
                                         _lib.NVFI_DEPTH_SKIP_HOLES if skip_holes else 0, float(loss_scale) * float(depth_weight),
                                         _lib.ptr(loss[_LOSS_DEPTH:]), _lib.ptr(g_depth), _lib.ptr(loss[_LOSS_DEPTH_COUNT:]), st))
        g_w = None
        if distortion_weight > 0.0:
            dbytes = _lib.bytes_of(L.nvfi_ray_distortion_workspace_bytes, R)
            dws = out[o_dw:]
            if dbytes > dws.numel() * 4:
                raise _lib.NvfiError(f"nvfi_ray_distortion wants a workspace of {dbytes} bytes, {dws.numel() * 4} were set aside")
            g_w = torch.empty(R, S, device=dev)
            _lib.check(L.nvfi_ray_distortion(R, S, _lib.ptr(weights), self.distortion_delta(), float(loss_scale) * distortion_weight, None,
                                             _lib.ptr(loss[_LOSS_DISTORTION:]), None, _lib.ptr(g_w), _lib.ptr(dws), dws.numel() * 4, st))
        flow_call = None
        if target_flow is not None:
            from ..utils import flow_loss as fl
            add = g_w is not None
            flow_call = fl.flow_loss_raw(desc, ws, flags, ray_o, ray_d, weights, t, flow_dt, flow_camera, target_flow, valid=flow_valid, kind=flow_kind,
                                         huber_delta=flow_huber_delta, grad_scale=float(loss_scale) * float(flow_weight), g_weights=g_w, add_gw=add,
                                         loss=loss[_LOSS_FLOW:_LOSS_FLOW + 2], flow2d=False, max_workspace_bytes=flow_max_workspace_bytes)
            g_w_flow = flow_call["g_weights"]
            self.last_flow_chunks, self.last_flow_workspace_bytes = flow_call["chunks"], flow_call["workspace"].numel()
        mask_call = None
        if target_mask is not None:
            from ..utils import mask_loss as ml
            g_prev = g_w if flow_call is None else g_w_flow
            md = _mask_desc(mask_field, mparams)
            mask_call = ml.mask_loss_raw(desc, md, ws, flags, weights, t, target_mask, kind=mask_kind, eps=mask_eps,
                                         grad_scale=float(loss_scale) * float(mask_weight), g_weights=g_prev, add_gw=g_prev is not None,
                                         loss=loss[_LOSS_MASK:_LOSS_MASK + 2], mask_map=None, max_workspace_bytes=mask_max_workspace_bytes)
            g_w_mask = mask_call["g_weights"]
            self.last_mask_map, self.last_mask_n = mask_call["mask_map"], loss[_LOSS_MASK + 1]
            self.last_mask_chunks, self.last_mask_workspace_bytes = mask_call["chunks"], mask_call["workspace"].numel()
        if wait_before_backward is not None:
            torch.cuda.current_stream().wait_stream(wait_before_backward)
        G = self._grads_struct_cached(ps)
        _lib.check(L.nvfi_render_bwd_t(C.byref(desc), R, _lib.ptr(ray_o), _lib.ptr(ray_d), t, int(t_dev is not None), flags, _lib.ptr(weights),
                                       _lib.ptr(g_rgb), _lib.ptr(g_depth), None,
                                       _lib.ptr(g_w_mask if mask_call is not None else g_w if flow_call is None else g_w_flow), C.byref(G),
                                       _lib.ptr(ws), ws.numel(), st))
        res = (loss[_LOSS_MSE], rgb) if g_depth is None else (loss[_LOSS_MSE], rgb, loss[_LOSS_DEPTH])
        if g_w is not None:
            res = res + (loss[_LOSS_DISTORTION],)
        if flow_call is not None:
            fl.flow_loss_backward_raw(desc, flow_call, G)
            res = res + (loss[_LOSS_FLOW],)
        if mask_call is not None:
            ml.mask_loss_backward_raw(md, mask_call, ml.mask_grads_struct([p.grad if p.requires_grad else None for p in mparams]))
            res = res + (loss[_LOSS_MASK],)
        return res

    def _mask_field_arg(self, mask_field, who):
        mask_field = self.mask_field if mask_field is None else mask_field
        if mask_field is None:
            raise ValueError(f"{who} needs a mask_field (the argument or self.mask_field)")
        if getattr(mask_field, "mfma_fp16", False):
            raise NotImplementedError(f"{who}: the fp16-input MaskField mode has no loss path (exact fp32 MFMA only)")
        return mask_field

    def mask_loss(self, weights, target, mask_field=None, kind="ce", eps=1e-5, weight_grad=True, max_workspace_bytes=1 << 30):
        """2-D mask supervision of a training render (include/nvfi_hip.h: nvfi_mask_loss_fwd / _bwd; utils/mask_loss.py) -> 0-dim loss with
        gradient.  `weights` must be the (R, S) tensor that a training `forward` of this field returned - the tensor itself, with its autograd
        node, whose workspace (masked list, warped positions) the call reads; anything else, or a render whose backward has already run,
        raises ValueError, a DeviceTime render NotImplementedError.  It need not be the most recent render.
        mask_map[r] = sum_j w_j softmax(mask_field(x_j)) over the render's appearance-masked samples (mask_field defaults to self.mask_field;
        the render need not have been made with it attached).  target: int (R) labels - [0, K) one-hot, K background, negative ignored - or
        float (R, K) rows (a row with a non-finite entry is ignored).  kind "l2": 1 / (2 n K) sum (mask_map - y)^2; "ce": -(1 / n) sum y
        log(mask_map + eps); n the number of rays that are not ignored.
        The gradient reaches the weights (and through the render backward everything the render depends on; weight_grad=False leaves the
        weights without gradient) and the ten MaskField parameters; the points carry none, no second order.  The backward splits the
        R * nSamples capacity of the masked list into chunks whose plan stays under max_workspace_bytes (self.last_mask_chunks,
        self.last_mask_workspace_bytes).  self.last_mask_map holds the (R, K) map, self.last_mask_n the device-side count of rays."""
        mask_field = self._mask_field_arg(mask_field, "mask_loss")
        if not (isinstance(weights, torch.Tensor) and weights.is_cuda):
            raise _lib.NvfiError("mask_loss needs the weights of a render on the GPU (no CPU fallback exists)")
        node = weights.grad_fn
        if not isinstance(node, _RenderFn._backward_cls) or getattr(node, "field", None) is not self or not (getattr(node, "flags", 0) & _lib.NVFI_TRAIN):
            raise ValueError("mask_loss: `weights` must be the tensor a training forward of this field returned (with its autograd node)")
        if node.ws is None:
            raise ValueError("mask_loss: the workspace of that render was released by its backward; call mask_loss before backward")
        if node.t_on_device:
            raise NotImplementedError("mask_loss: DeviceTime renders are not supported (the mask loss plans with a host-scalar time)")
        w_in = weights if (weight_grad and torch.is_grad_enabled()) else weights.detach()
        return _MaskLossFn.apply(self, w_in, node, mask_field, target, kind, float(eps), int(max_workspace_bytes), *mask_field._params())

    @torch.no_grad()
    def mask_fit_backward_(self, t, ray_o, ray_d, target_mask, mask_field=None, kind="ce", eps=1e-5, loss_scale=1.0, white_bg=True, jitter=None,
                           max_workspace_bytes=1 << 30, workspace=None):
        """The frozen-scene step of fitting a MaskField to 2-D masks of a trained scene: an eval-mode render of the rays (no training stash,
        no render backward), the mask loss of its masked samples with no weight gradient, and the chunked MaskField backward ACCUMULATED
        into the .grad of the mask field's ten parameters (which must exist), scaled by loss_scale.  Three library calls plus one per
        chunk; no torch launch and no host synchronisation when target_mask arrives as contiguous int32 labels or float32 (R, K) rows, so
        the step can be captured in a graph.  jitter (default None: the eval render's fixed samples and alpha-mask cull): a per-ray sample
        offset in [0, 1); the library jitters only renders flagged NVFI_TRAIN, so with a jitter the render is made in training mode - the
        training sampling rules, and a workspace that holds the training stash nobody reads.
        Workspace: the masked count stays on the device, so the plan covers the R * nSamples CAPACITY of the masked list - the largest chunk
        whose plan stays under max_workspace_bytes (default 1 GiB; 2 048 x 128 rays take all of it, in two chunks, whatever the count is:
        self.last_mask_chunks, self.last_mask_workspace_bytes).  A fit loop should lower max_workspace_bytes to a few chunks' worth and pass
        `workspace`, a uint8 device tensor of at least utils.mask_loss.mask_loss_plan(...)[1] bytes that it keeps across steps (nothing in
        it outlives the call); without it every call allocates the plan afresh.
        Returns (loss, mask_map): the UN-scaled 0-dim value and the (R, K) map; self.last_mask_n is the device-side count of rays."""
        from ..utils import mask_loss as ml
        L = _lib.lib()
        mask_field = self._mask_field_arg(mask_field, "mask_fit_backward_")
        if getattr(t, "dev", None) is not None:
            raise NotImplementedError("mask_fit_backward_: DeviceTime renders are not supported")
        mparams = mask_field._params()
        if any(p.requires_grad and (p.grad is None or not p.grad.is_contiguous()) for p in mparams):
            raise _lib.NvfiError("mask_fit_backward_ accumulates into the .grad of the mask field's parameters: they must exist")
        ray_o, ray_d, t = self._prep_rays(ray_o, ray_d, t)
        R = ray_o.shape[0]
        flags = _lib.NVFI_WHITE_BG if white_bg else 0
        if jitter is not None:
            flags |= _lib.NVFI_TRAIN
            jitter = jitter.reshape(-1).float().contiguous()
        desc, ws, (rgb, depth, acc, weights, counters) = self._ray_buffers(R, ray_o.device, t, flags)
        st = _stream_ptr()
        _lib.check(L.nvfi_render_fwd_t(C.byref(desc), R, _lib.ptr(ray_o), _lib.ptr(ray_d), _lib.ptr(jitter), t, None, flags, _lib.ptr(rgb),
                                       _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.ptr(counters), st))
        self.last_counters = counters
        md = _mask_desc(mask_field, mparams)
        call = ml.mask_loss_raw(desc, md, ws, flags, weights, t, target_mask, kind=kind, eps=eps, grad_scale=float(loss_scale), g_weights=False,
                                max_workspace_bytes=int(max_workspace_bytes), workspace=workspace)
        ml.mask_loss_backward_raw(md, call, ml.mask_grads_struct([p.grad if p.requires_grad else None for p in mparams]))
        self.last_mask_map, self.last_mask_n = call["mask_map"], call["loss"][1]
        self.last_mask_chunks, self.last_mask_workspace_bytes = call["chunks"], call["workspace"].numel()
        return call["loss"][0], call["mask_map"]

    def flow_loss(self, weights, dt, camera, target_flow, valid=None, kind="l2", huber_delta=1.0, weight_grad=True, max_workspace_bytes=1 << 30):
        """Optical-flow supervision of a training render (include/nvfi_hip.h: nvfi_flow_loss_fwd / _bwd; utils/flow_loss.py) -> 0-dim loss
        with gradient.  `weights` must be the (R, S) tensor that a training `forward` of this field returned - the tensor itself, with its
        autograd node, whose workspace (masked list, sample depths) the call reads; anything else, or a render whose backward has already run,
        raises ValueError.  It need not be the most recent render: every render owns its workspace until its backward.  A render made with a
        mask_field attached (the mask branch) raises NotImplementedError, as in render_mse_backward_.
        flow2d[r] = sum_j w_j (pi(integrate_pos(x_j, t, t + dt)) - pi(x_j)) over the render's appearance-masked samples, pi the projection of
        `camera` ((pose3x4, H, W, focal) or an object with pose / height / width / focal); loss = (1 / (2 n)) sum over the n valid rays (valid[r]
        != 0 and a finite target) and both components of (flow2d - target_flow)^2 (kind="l2") or of torch's huber element (kind="huber").
        The gradient reaches the weights (and through the render backward everything the render depends on; weight_grad=False leaves the
        weights without gradient) and the 12 tensors of vel_net.weight_net through the adjoint of integrate_pos, every gate / rejection / guard
        decision held fixed; nothing else, no second order.  The backward splits the R * nSamples capacity of the masked list into chunks
        whose plan stays under max_workspace_bytes (self.last_flow_chunks, self.last_flow_workspace_bytes); the workspace lives from this call
        to its backward.  self.last_flow2d holds the (R, 2) flow map, self.last_flow_n the device-side count of valid rays."""
        if not self.use_vel:
            raise _lib.NvfiError("flow_loss needs a field with a velocity net (use_vel)")
        if not (isinstance(weights, torch.Tensor) and weights.is_cuda):
            raise _lib.NvfiError("flow_loss needs the weights of a render on the GPU (no CPU fallback exists)")
        node = weights.grad_fn
        if not isinstance(node, _RenderFn._backward_cls) or getattr(node, "field", None) is not self or not (getattr(node, "flags", 0) & _lib.NVFI_TRAIN):
            raise ValueError("flow_loss: `weights` must be the tensor a training forward of this field returned (with its autograd node)")
        if node.flags & _lib.NVFI_WANT_MASK:
            raise NotImplementedError("flow_loss: renders of the mask branch (a mask_field attached) are not supported")
        if node.ws is None:
            raise ValueError("flow_loss: the workspace of that render was released by its backward; call flow_loss before backward")
        if node.t_on_device:
            raise NotImplementedError("flow_loss: DeviceTime renders are not supported (the flow loss plans with a host-scalar time)")
        wparams = self._render_params()[fs.WEIGHT_NET]
        w_in = weights if weight_grad else weights.detach()
        if not torch.is_grad_enabled():
            w_in = weights.detach()
        return _FlowLossFn.apply(self, w_in, node, float(dt), camera, target_flow, valid, kind, float(huber_delta), int(max_workspace_bytes), *wparams)

    def distortion_delta(self):
        """width of one sample interval in normalised ray distance s = (z - near) / (far - near): stepSize / (far - near), the `delta` of
        the distortion loss (every built sampling path spaces a ray's samples by stepSize)"""
        return float(self._step_host) / (float(self.near_far[1]) - float(self.near_far[0]))

    def distortion_loss(self, weights):
        """utils.ray_regs.distortion_loss(weights, self.distortion_delta()): the (R, S) weights of a training render -> 0-dim loss with gradient"""
        from ..utils.ray_regs import distortion_loss
        return distortion_loss(weights, self.distortion_delta())

    def _jitter(self, R, device):
        """Per-ray jitter drawn on the CPU generator like the reference (tensorf_base.py:302-306), staged through a small
        ring of pinned buffers so the upload is asynchronous."""
        ov = self.__dict__.get("jitter_override")
        if ov is not None:       # tests: explicit per-ray jitter instead of a draw
            return ov.to(device).reshape(-1).float().contiguous()
        ring = _rt(self).setdefault("_jit_ring", [])      # entries: [pinned buffer, event recorded after its last upload]
        idx = _rt(self).get("_jit_idx", 0)
        if len(ring) < 4:
            ring.append([torch.empty(max(R, 4096), 1).pin_memory(), None])
        slot = ring[idx % len(ring)]
        if slot[1] is not None:
            slot[1].synchronize()      # the asynchronous copy that last read this buffer must have executed before it is rewritten
        if slot[0].shape[0] < R:
            slot[0] = torch.empty(R, 1).pin_memory()
        _rt(self)["_jit_idx"] = idx + 1
        view = slot[0][:R]
        torch.rand(R, 1, out=view)
        out = view.to(device, non_blocking=True).reshape(-1)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        return out

    def _scratch(self, key, nbytes, device):
        """Reusable workspace for calls whose workspace does not have to outlive the call."""
        cache = _rt(self).setdefault("_scratch_cache", {})
        buf = cache.get(key)
        if buf is None or buf.numel() < nbytes or buf.device != device:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            cache[key] = buf
        return buf

    # ------------------------------------------------------------------ per-iteration regularisers (next-row f-1; torch ops)
    def _reg_planes(self):
        return list(self.density_plane_space) + list(self.density_plane_time) + list(self.app_plane_space)

    def _reg_on_device(self, reg=None):
        from ..utils.tensorf_utils import is_reference_tvloss
        return self.aabb.is_cuda and not self.__dict__.get("regs_torch_ops", False) and self.density_n_comp[0] % 4 == 0 and self.app_n_comp[0] % 4 == 0 and (reg is None or is_reference_tvloss(reg))

    def density_L1(self):
        if self._reg_on_device():
            return _RegFn.apply(self, 0, *self._reg_planes())
        total = 0
        for i in range(3):
            total = total + torch.mean(torch.abs(self.density_plane_space[i])) + torch.mean(torch.abs(1 - self.density_plane_time[i]))
        return total

    def TV_loss_density(self, reg):
        if self._reg_on_device(reg):
            return _RegFn.apply(self, 1, *self._reg_planes()) * reg.TVLoss_weight
        total = 0
        for i in range(3):
            total = total + reg(self.density_plane_space[i]) * 1e-2 + ((reg(self.density_plane_time[i], t=True) * 1e-2) if self.num_keyframes > 1 else 0)
        return total

    def TV_loss_app(self, reg):
        if self._reg_on_device(reg):
            return _RegFn.apply(self, 2, *self._reg_planes()) * reg.TVLoss_weight
        total = 0
        for i in range(3):
            total = total + reg(self.app_plane_space[i]) * 1e-2
        return total

    @torch.no_grad()
    def regularizers_backward_(self, w_l1, w_tv_density=None, w_tv_app=None):
        """Fused form of `loss += w_l1*density_L1() + w_tv_density*TV_loss_density(reg) + w_tv_app*TV_loss_app(reg)`
        followed by backward: one pass per plane that ACCUMULATES the weighted gradients into p.grad and returns the
        three un-weighted loss values (device tensor [L1, TVd, TVa]).  Call it next to loss.backward()."""
        L = _lib.lib()
        ps = self._render_params()[fs.REG]
        grads, _ = self._grad_targets(ps, [True] * len(ps), mode=True)
        for g, p in zip(grads, ps):
            if g.stride() != p.stride():
                raise _lib.NvfiError("plane .grad must share the channels_last layout of its parameter")
        G = self._grads_struct(fs.at(fs.REG, grads))
        out = torch.empty(3, device=ps[0].device)
        desc = self._desc()
        if isinstance(w_l1, torch.Tensor):       # the three weights as one fp32[3] CUDA tensor (hipGraph replay: they decay every iteration)
            if not (w_l1.is_cuda and w_l1.dtype == torch.float32 and w_l1.numel() == 3 and w_l1.is_contiguous()):
                raise _lib.NvfiError("device-side regulariser weights must be a contiguous fp32[3] CUDA tensor")
            _lib.check(L.nvfi_plane_regs_dev(C.byref(desc), _lib.ptr(w_l1), _lib.ptr(out), C.byref(G), _stream_ptr()))
            return out
        _lib.check(L.nvfi_plane_regs(C.byref(desc), w_l1, w_tv_density, w_tv_app, _lib.ptr(out),
                                     C.byref(G), _stream_ptr()))
        return out

    # ------------------------------------------------------------------ optimiser / checkpoint surface
    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001):
        """tensorf_keyframe.py:539-550"""
        gv = [{"params": self.density_plane_space, "lr": lr_init_spatialxyz},
              {"params": self.density_plane_time, "lr": lr_init_spatialxyz},
              {"params": self.app_plane_space, "lr": lr_init_spatialxyz},
              {"params": self.app_plane_time, "lr": lr_init_spatialxyz},
              {"params": self.basis_mat.parameters(), "lr": lr_init_network},
              {"params": self.basis_mat_density.parameters(), "lr": lr_init_network}]
        if isinstance(self.renderModule, nn.Module):
            gv += [{"params": self.renderModule.parameters(), "lr": lr_init_network}]
        if self.use_vel:
            gv += [{"params": self.vel.parameters(), "lr": lr_init_network}]
        return gv

    def get_kwargs(self):
        """tensorf_base.py:247-268"""
        kw = {"aabb": self.aabb, "gridSize": self.gridSize.tolist(), "density_n_comp": self.density_n_comp,
              "appearance_n_comp": self.app_n_comp, "app_dim": self.app_dim, "density_shift": self.density_shift,
              "alphaMask_thres": self.alphaMask_thres, "fea2denseAct": self.fea2denseAct, "near_far": self.near_far,
              "step_ratio": self.step_ratio, "shadingMode": self.shadingMode, "pos_pe": self.pos_pe, "view_pe": self.view_pe,
              "fea_pe": self.fea_pe, "featureC": self.featureC, "num_keyframes": self.num_keyframes}
        if self.alphaMask is not None:
            kw["alphaMask_grid"] = self.alphaMask.gridSize
        return kw

    # ------------------------------------------------------------------ occupancy grid maintenance (next-row f-3)
    @torch.no_grad()
    def compute_alpha(self, xyzt_locs, length=0.01, times=None, time_offset=None, transfer=False):
        """tensorf_keyframe.py:508-537 with per-point times (xyzt_locs[..., 3] raw t, [..., :3] world xyz)."""
        pts = self.normalize_coord(xyzt_locs[..., :3].reshape(-1, 3))
        t = xyzt_locs[..., -1:].reshape(-1, 1).float()
        ts = self.tmax / (self.num_keyframes - 1) if self.num_keyframes > 1 else 1
        base = torch.zeros_like(t) if transfer else torch.round((t / ts).clamp(0.0, self.num_keyframes - 1)) * ts
        prev = self.integrate_pos(pts, t, base) if self.use_vel else pts
        feat = self.compute_densityfeature(torch.cat([prev, self.normalize_time_coord(base)], dim=-1))
        sigma = self.feature2density(feat, {})
        return (1 - torch.exp(-sigma * length)).view(xyzt_locs.shape[:-1])

    @torch.no_grad()
    def getDenseAlpha(self, gridSize=None, transfer=False):
        """tensorf_keyframe.py:461-499: running maximum of alpha over the 60 frame times i/60 on a dense grid."""
        L = _lib.lib()
        dev = self.aabb.device
        samples = torch.stack(torch.meshgrid(torch.linspace(0, 1, gridSize[0]), torch.linspace(0, 1, gridSize[1]),
                                             torch.linspace(0, 1, gridSize[2]), indexing="ij"), -1).to(dev)
        dense_xyz = self.aabb[0] * (1 - samples) + self.aabb[1] * samples
        flat = dense_xyz.reshape(-1, 3).contiguous()
        N = flat.shape[0]
        alpha = torch.zeros(N, device=dev)
        desc = self._desc()
        nb = _lib.bytes_of(L.nvfi_alpha_workspace_bytes, C.byref(desc), N)
        ws = self._scratch("alpha", nb, dev)
        for t in (np.linspace(0, 59, 60) / 60):
            _lib.check(L.nvfi_compute_alpha(C.byref(desc), N, _lib.ptr(flat), float(np.float32(t)), int(transfer), self._step_host, 1,
                                            _lib.ptr(alpha), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        return alpha.view(gridSize[0], gridSize[1], gridSize[2]), dense_xyz

    @torch.no_grad()
    def updateAlphaMask(self, gridSize=(200, 200, 200), transfer=False):
        """tensorf_keyframe.py:379-405: dilate (3^3 max-pool), threshold, build the AlphaGridMask, return the tight aabb."""
        gridSize = [int(g) for g in gridSize]
        alpha, dense_xyz = self.getDenseAlpha(gridSize, transfer=transfer)
        dense_xyz = dense_xyz.transpose(0, 2).contiguous()
        alpha = alpha.clamp(0, 1).transpose(0, 2).contiguous()[None, None]
        alpha = F.max_pool3d(alpha, kernel_size=3, padding=1, stride=1).view(gridSize[::-1])
        alpha[alpha >= self.alphaMask_thres] = 1
        alpha[alpha < self.alphaMask_thres] = 0
        self.alphaMask = AlphaGridMask(self.aabb.device, self.aabb, alpha)
        valid_xyz = dense_xyz[alpha > 0.5]
        return torch.stack((valid_xyz.amin(0), valid_xyz.amax(0)))

    @torch.no_grad()
    def shrink(self, new_aabb):
        """tensorf_keyframe.py:407-458: crop every plane to the voxel range of new_aabb."""
        xyz_min, xyz_max = new_aabb
        t_l, b_r = (xyz_min - self.aabb[0]) / self.units, (xyz_max - self.aabb[0]) / self.units
        t_l, b_r = torch.round(torch.round(t_l)).long(), torch.round(b_r).long() + 1
        b_r = torch.stack([b_r, self.gridSize]).amin(0)
        tl, br = t_l.tolist(), b_r.tolist()

        def crop(space, time):
            ns, nt = [], []
            for i in range(3):
                a, b = self.matModeSpace[i]
                c = self.matModeTime[i][0]
                ns.append(nn.Parameter(_cl(space[i].data[..., tl[b]:br[b], tl[a]:br[a]].clone())))
                nt.append(nn.Parameter(_cl(time[i].data[..., :, tl[c]:br[c]].clone())))
            return nn.ParameterList(ns), nn.ParameterList(nt)

        self.density_plane_space, self.density_plane_time = crop(self.density_plane_space, self.density_plane_time)
        self.app_plane_space, self.app_plane_time = crop(self.app_plane_space, self.app_plane_time)
        if self.alphaMask is not None and not torch.all(self.alphaMask.gridSize == self.gridSize):
            t_l_r, b_r_r = t_l / (self.gridSize - 1), (b_r - 1) / (self.gridSize - 1)
            correct = torch.zeros_like(new_aabb)
            correct[0] = (1 - t_l_r) * self.aabb[0] + t_l_r * self.aabb[1]
            correct[1] = (1 - b_r_r) * self.aabb[0] + b_r_r * self.aabb[1]
            new_aabb = correct
        newSize = b_r - t_l
        self.aabb.copy_(new_aabb)       # the surround-box gate keeps the INITIAL aabb (velocity_field.py:44 quirk)
        self.update_stepSize([int(v) for v in newSize.tolist()])

    # ------------------------------------------------------------------ grid maintenance (next-row f-3; torch ops)
    @torch.no_grad()
    def upsample_volume_grid(self, res_target, new_keyframes):
        """tensorf_keyframe.py:327-376: bilinear align_corners=True resampling of every plane."""
        self.num_keyframes = new_keyframes
        self.time_scale_factor = self.tmax / (self.num_keyframes - 1) if self.num_keyframes > 1 else 1

        def up(space, time):
            ns, nt = [], []
            for i in range(3):
                a, b = self.matModeSpace[i]
                c = self.matModeTime[i][0]
                ns.append(nn.Parameter(_cl(F.interpolate(space[i].data, size=(int(res_target[b]), int(res_target[a])), mode="bilinear", align_corners=True))))
                nt.append(nn.Parameter(_cl(F.interpolate(time[i].data, size=(self.num_keyframes, int(res_target[c])), mode="bilinear", align_corners=True))))
            return nn.ParameterList(ns), nn.ParameterList(nt)

        self.app_plane_space, self.app_plane_time = up(self.app_plane_space, self.app_plane_time)
        self.density_plane_space, self.density_plane_time = up(self.density_plane_space, self.density_plane_time)
        self.update_stepSize(res_target)
