"""NVFi wrapper (reference models/nvfi.py:17-84): builds the field, render_ray[_transfer], PDE regulariser."""
import torch
import torch.nn as nn

from .tensorf_keyframe import TensorVMKeyframeTimeKplane

_MODELS = {"TensorVMKeyframeTimeKplane": TensorVMKeyframeTimeKplane}


def _aslist(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


class NVFi(nn.Module):
    def __init__(self, config, device, aabb, res_cur, near_far):
        super().__init__()
        self.config = config.nvfi
        if self.config.model_name not in _MODELS:
            raise NotImplementedError(f"model_name {self.config.model_name}: only TensorVMKeyframeTimeKplane is reachable in the reference")
        self.nvfi = _MODELS[self.config.model_name](aabb, res_cur, device, near_far=near_far, cfg=config.nvfi)

    def train(self, mode=True):
        """train_nvfi.py:141-142 calls nvfi.train(); renderer.train() every iteration; walking ~180 sub-modules twice per step is 0.7 ms
        of pure host time, so an unchanged mode returns at once.  "Unchanged" is checked on this module, on the field and on the field's
        direct children (tests and drivers call model.nvfi.eval() / .train() on the inner field, and mask_field / alphaMask are attached
        later): a handful of attribute reads, not the 180-module walk; every 64th call does the full walk."""
        mode = bool(mode)
        d = self.__dict__
        # (a grandchild toggled on its own - model.nvfi.vel_net.weight_net.eval() - is below what the fast check sees: every 64th call walks
        # the whole tree anyway, 0.7 ms / 64 per step)
        d["_mode_calls"] = n = d.get("_mode_calls", 0) + 1
        if self.training == mode and d.get("_mode_walked") == mode and (n & 63):
            f = self._modules.get("nvfi")
            if f is None or (f.training == mode and all(c.training == mode for c in f._modules.values() if c is not None)):
                return self
        super().train(mode)
        d["_mode_walked"] = mode
        return self

    def render_ray(self, t, ray_o, ray_d, white_bg=True, ndc_ray=False):
        return self.nvfi(t, ray_o, ray_d, white_bg, ndc_ray)

    def render_ray_transfer(self, t, ray_o, ray_d, white_bg=True, ndc_ray=False):
        return self.nvfi(t, ray_o, ray_d, white_bg, ndc_ray, transfer_vel=True)

    def render_ray_flow(self, t, ray_o, ray_d, dt, camera=None, white_bg=True, transfer_vel=False):
        """eval-mode render with the velocity, scene-flow and optical-flow maps (TensorVMKeyframeTimeKplane.render_flow)"""
        return self.nvfi.render_flow(t, ray_o, ray_d, dt, camera=camera, white_bg=white_bg, transfer_vel=transfer_vel)

    def render_ray_objects(self, t, ray_o, ray_d, select=None, white_bg=True, transfer_vel=False):
        """eval-mode render with the per-object layers of the mask field, optionally object-selected (TensorVMKeyframeTimeKplane.render_objects)"""
        return self.nvfi.render_objects(t, ray_o, ray_d, select=select, white_bg=white_bg, transfer_vel=transfer_vel)

    def advect(self, pos, t, t_target, max_workspace_bytes=1 << 30):
        """integrate_pos(pos, t, t_target) with gradients to `pos` and the velocity net (TensorVMKeyframeTimeKplane.advect)"""
        return self.nvfi.advect(pos, t, t_target, max_workspace_bytes=max_workspace_bytes)

    def advect_pt(self, pos, t, t_target, max_workspace_bytes=1 << 30):
        """`advect` with per-point times: `t` / `t_target` a float or a device tensor of N elements each (TensorVMKeyframeTimeKplane.advect_pt)"""
        return self.nvfi.advect_pt(pos, t, t_target, max_workspace_bytes=max_workspace_bytes)

    def lookup_density(self, xyzt):
        """compute_densityfeature with gradients to the points and the density planes (TensorVMKeyframeTimeKplane.lookup_density)"""
        return self.nvfi.lookup_density(xyzt)

    def lookup_appfeature(self, xyzt):
        """compute_appfeature with gradients to the points, the appearance planes and basis_mat (TensorVMKeyframeTimeKplane.lookup_appfeature)"""
        return self.nvfi.lookup_appfeature(xyzt)

    def compute_appfeature(self, xyzt):
        """compute_appfeature, forward only (TensorVMKeyframeTimeKplane.compute_appfeature)"""
        return self.nvfi.compute_appfeature(xyzt)

    def shade(self, pts, viewdirs, features, max_workspace_bytes=1 << 30):
        """renderModule(pts, viewdirs, features) with gradients to all three and to renderModule.mlp (TensorVMKeyframeTimeKplane.shade)"""
        return self.nvfi.shade(pts, viewdirs, features, max_workspace_bytes=max_workspace_bytes)

    def lookup_rgb(self, xyzt, viewdirs, max_workspace_bytes=1 << 30):
        """the colour of given points with gradients to the points, the appearance planes, basis_mat and the MLP (TensorVMKeyframeTimeKplane.lookup_rgb)"""
        return self.nvfi.lookup_rgb(xyzt, viewdirs, max_workspace_bytes=max_workspace_bytes)

    def distortion_delta(self):
        """stepSize / (far - near): the interval width the distortion loss takes (TensorVMKeyframeTimeKplane.distortion_delta)"""
        return self.nvfi.distortion_delta()

    def distortion_loss(self, weights):
        """distortion loss of the (R, S) ray weights of a training render, with gradient (TensorVMKeyframeTimeKplane.distortion_loss)"""
        return self.nvfi.distortion_loss(weights)

    def flow_loss(self, weights, dt, camera, target_flow, **kw):
        """optical-flow supervision of a training render, with gradient (TensorVMKeyframeTimeKplane.flow_loss)"""
        return self.nvfi.flow_loss(weights, dt, camera, target_flow, **kw)

    def mask_loss(self, weights, target, **kw):
        """2-D mask supervision of a training render, with gradient (TensorVMKeyframeTimeKplane.mask_loss)"""
        return self.nvfi.mask_loss(weights, target, **kw)

    def update_nvfi_kwargs(self, kwargs):
        """models/nvfi.py:33-35 writes every checkpoint kwarg into the field's __dict__.  Same effect here, except that the two
        entries the C-ABI descriptor caches on the host (aabb, gridSize) go through the buffer / update_stepSize."""
        f = self.nvfi
        # the reference only rewrites __dict__ entries: a checkpoint whose STRUCTURAL kwargs differ from the constructed module (render
        # module kind, feature widths) would leave its renderModule / basis_mat as built and silently disagree with the descriptor the
        # kernels read, so such a checkpoint is refused here instead (build the model from the checkpoint's own config, train_nvfi.py:372-377)
        for k in ("shadingMode", "app_dim", "pos_pe", "view_pe", "fea_pe", "featureC", "density_n_comp", "appearance_n_comp", "num_keyframes"):
            have = getattr(f, "app_n_comp" if k == "appearance_n_comp" else k, None)
            if k in kwargs and have is not None and list(_aslist(kwargs[k])) != list(_aslist(have)):
                raise ValueError(f"update_nvfi_kwargs: checkpoint {k}={kwargs[k]!r} but the module was built with {have!r}")
        for k, v in kwargs.items():
            if k == "aabb":
                f.aabb.copy_(torch.as_tensor(v).to(f.aabb.device))
            elif k == "gridSize":
                continue
            elif k == "appearance_n_comp":
                f.app_n_comp = v
            elif k == "alphaMask_grid":
                f.__dict__[k] = v
            else:
                setattr(f, k, v)
        f.update_stepSize([int(g) for g in kwargs.get("gridSize", f.gridSize.tolist())])

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001, lr_init_velocity=0.001):
        return self.nvfi.get_optparam_groups(lr_init_spatialxyz, lr_init_network)

    def get_vel_loss(self, n_pts=32768., points=None, t=None):
        """Velocity PDE regulariser (nvfi.py:42-84).  Collocation points are drawn on the device generator
        exactly like the reference unless given explicitly.  Returns python 0. when no point is occupied."""
        f = self.nvfi
        if points is None:
            mn, mx = f.aabb
            points = torch.rand(int(n_pts), 3, device=f.aabb.device) * (mx - mn) + mn
            t = torch.rand(int(n_pts), 1, device=f.aabb.device)
        if f.accumulate_grads_inplace is True and torch.is_grad_enabled() and getattr(self, "vel_loss_weight", None) is not None:
            # fused value + backward: gradients of vel_loss_weight * loss go straight into .grad
            # (sync-free: the value is a 0-dim tensor, 0.0 when no point is occupied - the reference's python `0.` would need the count on the host)
            out = f.pde_loss_backward_(points, t, self.vel_loss_weight, getattr(self, "vel_grad_targets", None))
            return out[0]
        loss = f.pde_loss(points, t)
        if f.last_pde_n_kept == 0:   # known on the host from the call's one internal sync (`xyzt.shape[0] == 0` in the reference)
            return 0.
        return loss
