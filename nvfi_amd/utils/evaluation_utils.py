"""Checkpoint compatibility (next-row f-4): same dictionary layout and file naming as the reference
(train_nvfi.py:359-392, utils/evaluation_utils.py:20-43), so checkpoints interchange between the two implementations."""
import glob
import os

import torch


def save_checkpoint(path, nvfi, optimizer, epoch=None):
    """{logdir}/model_{epoch:05d}.ckpt with keys model_state_dict / optimizer_state_dict / nvfi_kwarg (train_nvfi.py:359-369).
    Planes are saved with their logical (1,C,H,W) shape; the channels_last physical layout is an implementation detail."""
    sd = {k: (v.contiguous() if v.dim() == 4 else v) for k, v in nvfi.state_dict().items()}
    ckpt = {"model_state_dict": sd, "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else {},
            "nvfi_kwarg": nvfi.nvfi.get_kwargs()}
    if epoch is not None:
        path = os.path.join(path, "model_%05d.ckpt" % epoch)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save(ckpt, path)
    return path


def load_checkpoint(logdir, map_location="cpu"):
    """newest *.ckpt under logdir (utils/evaluation_utils.py:20-43)"""
    files = sorted(glob.glob(os.path.join(logdir, "*.ckpt")))
    if not files:
        raise FileNotFoundError(f"no checkpoint under {logdir}")
    return torch.load(files[-1], map_location=map_location, weights_only=False)


def load_model_checkpoint(cfg, ckpt, device):
    """Rebuild NVFi at the saved aabb / gridSize / num_keyframes and load the weights (train_nvfi.py:372-392)."""
    from ..models import NVFi, Renderer, AlphaGridMask
    kw = ckpt["nvfi_kwarg"]
    cfg.nvfi.num_keyframes = kw["num_keyframes"]
    # near / far come from the dataset section like the reference (:375); the checkpoint's kwargs then override attributes (:378)
    near_far = [cfg.dataset.near, cfg.dataset.far] if "dataset" in cfg else kw["near_far"]
    nvfi = NVFi(cfg, device, kw["aabb"].to(device), kw["gridSize"], near_far).to(device)
    nvfi.update_nvfi_kwargs(kw)
    sd = ckpt["model_state_dict"]
    if "nvfi.alphaMask.alpha_aabb" in sd and "nvfi.alphaMask.alpha_volume" in sd:      # the occupancy mask is rebuilt first (:380-385)
        nvfi.nvfi.alphaMask = AlphaGridMask(device, sd["nvfi.alphaMask.alpha_aabb"].to(device), sd["nvfi.alphaMask.alpha_volume"].to(device))
    nvfi.load_state_dict(sd)            # strict: a missing or unexpected key is an error, as in the reference (:386)
    renderer = Renderer(nvfi, cfg.renderer.batch_size, cfg.renderer.test_batch_size, cfg.renderer.n_rays,
                        cfg.renderer.distance_scale, tensorf_sample=cfg.renderer.tensorf_sample, ndc=cfg.renderer.ndc) if "renderer" in cfg else None
    return nvfi, renderer


def depth_loss_raw(pred, gt, gt_index=None, skip_holes=False, grad_scale=1.0, out=None, check_index=True):
    """One nvfi_depth_loss launch (include/nvfi_hip.h) on flat fp32 device tensors, nothing else: -> (loss, g_pred, n_counted), a 0-dim
    tensor with the UN-scaled loss, grad_scale * d(loss)/d(pred) (n,) and a 0-dim int64 tensor with the number of counted entries.
    gt_index (int64, n): the target of entry i is gt[gt_index[i]].  The kernel does not range-check the indices, so this function does
    (check_index=True: one min / max over the indices and a wait for it; an index outside gt raises IndexError before anything is launched).
    check_index=False leaves that out - no torch launch, no wait - for indices that are known to be in range, and inside a hipGraph capture.
    out: the three tensors to write into."""
    from .. import _lib
    if not (pred.is_cuda and gt.is_cuda and (gt_index is None or gt_index.is_cuda)):
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or not pred.is_contiguous() or not gt.is_contiguous():
        raise ValueError("depth_loss_raw takes contiguous float32 tensors")
    n = pred.numel()
    if gt_index is not None:
        if gt_index.dtype != torch.int64 or not gt_index.is_contiguous() or gt_index.numel() != n:
            raise ValueError(f"gt_index must be a contiguous int64 tensor of {n} entries")
        if check_index and n:
            lo, hi = (int(v) for v in torch.aminmax(gt_index))
            if lo < 0 or hi >= gt.numel():
                raise IndexError(f"gt_index holds {lo if lo < 0 else hi}, outside the {gt.numel()} entries of gt")
    elif gt.numel() != n:
        raise ValueError(f"pred has {n} entries, gt {gt.numel()}")
    if out is None:
        out = (torch.empty((), device=pred.device), torch.empty(n, device=pred.device), torch.empty((), dtype=torch.int64, device=pred.device))
    loss, g_pred, n_counted = out
    _lib.check(_lib.lib().nvfi_depth_loss(n, _lib.ptr(pred), _lib.ptr(gt), _lib.ptr(gt_index),
                                          _lib.NVFI_DEPTH_SKIP_HOLES if skip_holes else 0, float(grad_scale),
                                          _lib.ptr(loss), _lib.ptr(g_pred), _lib.ptr(n_counted), _lib.stream_ptr()))
    return loss, g_pred, n_counted


class _DepthLossFn(torch.autograd.Function):
    """value and gradient from one launch (nvfi_depth_loss, grad_scale = 1); backward is one scaling launch (the pattern of tensorf_utils._MseFn)"""

    @staticmethod
    def forward(ctx, pred, gt, skip_holes):
        shape = pred.shape
        loss, g_pred, _ = depth_loss_raw(pred.detach().reshape(-1).contiguous().float(), gt.detach().reshape(-1).contiguous().float(),
                                         skip_holes=skip_holes)
        ctx.save_for_backward(g_pred)
        ctx.shape, ctx.dtype = shape, pred.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (g_pred,) = ctx.saved_tensors
        return (g_pred * g).reshape(ctx.shape).to(ctx.dtype), None, None


def compute_depth_loss(pred, gt, skip_holes=False):
    """The reference's compute_depth_loss(pred, gt) (utils/evaluation_utils.py:8-17) on the GPU: each map is shifted by its median
    (torch.median: the LOWER median) and scaled by its mean absolute deviation (+ 1e-6), the loss is the MSE of the normalised maps.  Any
    shape, flattened; pred and gt must have the same number of entries.  One kernel launch forward (csrc/depthloss.hip, value and gradient),
    one scaling launch backward.  The gradient follows torch autograd, including its rule for the median (spread equally over all entries
    equal to it - every ray that hits nothing has depth == far).  Only `pred` receives a gradient: a `gt` that requires grad raises
    NotImplementedError.  skip_holes=True counts entry i only if gt[i] is finite and > 0 (sensor depth maps mark missing pixels with 0);
    the other entries get a gradient of exactly 0, and with nothing counted the loss is 0.  There is no CPU path: CPU tensors raise NvfiError.

    The drop-in form `loss = mse + w * compute_depth_loss(depth_map, target_dpts)` works with the depth map of a training render (its
    backward takes the depth gradient); the fused driver form is TensorVMKeyframeTimeKplane.render_mse_backward_(..., target_depth=).
    Multi-GPU: every rank normalises its OWN shard of the batch (its own medians and deviations); there is no global median."""
    from .. import _lib
    if gt.requires_grad:
        raise NotImplementedError("`gt` requires grad: only `pred` receives a gradient")
    if not pred.is_cuda or not gt.is_cuda:
        raise _lib.NvfiError("NVFi HIP kernels need tensors on the GPU (no CPU fallback exists)")
    if pred.numel() != gt.numel():
        raise ValueError(f"pred has {pred.numel()} entries, gt {gt.numel()}")
    return _DepthLossFn.apply(pred, gt, bool(skip_holes))


def render_test_evaluation(nvfi, renderer, poses, times, targets, H, W, focal, near, far, white_background=True,
                           savedir=None, update_alpha_mask=True, device=None, with_ssim=False, with_flow=None, gt_depths=None,
                           with_distortion=False, gt_flows=None, flow_dt=None, flow_valid=None):
    """Eval driver (train_nvfi.py:395-459 without the dataset / wandb plumbing): optional `updateAlphaMask` at the current grid
    (`:413`), one `Renderer.render(mode='test')` per (pose, time) frame (`:437`), 8-bit PNGs named r_%03d.png (`:449-451`,
    written with PIL - imageio is not a dependency here) and per-frame / mean PSNR against `targets` (H,W,3 in [0,1]).

    Returns {"psnr": [..], "mean_psnr": float, "images": uint8 array (N,H,W,3)}.  with_ssim=True adds "ssim": [..] and "mean_ssim": the SSIM of
    every frame against its target (utils.metrics.ssim_frames: the kernel reads the (H,W,3) frames in place; the values come to the host once,
    after the loop).  with_flow=dt (default off) renders every frame through Renderer.render_flow instead - same rgb - and adds "flow2d"
    (N,H,W,2), the optical flow over dt in pixels; with `savedir` its colour coding (utils.flow_vis.flow_to_rgb) is written as r_%03d_flow.png.
    gt_depths (default off: N depth frames (H,W), 0 / inf / NaN where the sensor saw nothing) adds "depth_loss": [..] and "mean_depth_loss": the
    median-normalised depth loss of every rendered depth map against its frame (compute_depth_loss with skip_holes=True: one launch per frame
    on the 640 000 entries of an 800 x 800 frame; the values come to the host once, after the loop).
    with_distortion=True adds "distortion": [..] and "mean_distortion", the distortion loss of every frame's ray weights
    (utils.ray_regs.distortion_loss_raw with the field's distortion_delta(): one call per frame), and "distortion_maps" (N,H,W), its per-pixel
    value D_r: a floater map - a frame whose mean jumps has a floater, the map shows where.
    gt_flows (default off: N target flow frames (H,W,2) in pixels over flow_dt, which must be given and takes the place of with_flow; flow_valid
    optional N masks (H,W), non-finite targets never count) renders every frame through Renderer.render_flow and adds "epe": [..] and
    "mean_epe", the end-point error of every frame: the mean of |flow2d - gt|_2 over its valid pixels (NaN for a frame without one); torch ops
    on the device, the values come to the host once, after the loop."""
    import numpy as np
    from ..models import Camera
    from .metrics import mse2psnr, ssim_frames
    device = device or next(nvfi.parameters()).device
    nvfi.eval()
    if update_alpha_mask:
        nvfi.nvfi.updateAlphaMask(nvfi.nvfi.gridSize)
    imgs, psnrs, ssims, flows, dlosses, dists, dmaps, epes = [], [], [], [], [], [], [], []
    if gt_flows is not None:
        if flow_dt is None:
            raise ValueError("gt_flows needs flow_dt, the time span the target flow covers")
        if with_flow is not None and float(with_flow) != float(flow_dt):
            raise ValueError(f"with_flow={with_flow} and flow_dt={flow_dt} disagree: one flow map is rendered per frame")
        with_flow = flow_dt
    if with_distortion:
        from .ray_regs import distortion_loss_raw
        delta = nvfi.distortion_delta()
    with torch.no_grad():
        for idx in range(len(poses)):
            pose = torch.as_tensor(poses[idx], dtype=torch.float32, device=device)
            cam = Camera(pose, H, W, focal, None, near, far)
            if with_flow is None:
                res = renderer.render(float(times[idx]), cam.rays.to(device), white_background=white_background, mode="test")
                rgb = res[0]
            else:
                res = renderer.render_flow(float(times[idx]), cam.rays.to(device), float(with_flow), camera=cam, white_background=white_background)
                rgb = res[0]
                flows.append(res[6].reshape(H, W, 2))
                if gt_flows is not None:
                    gt = torch.as_tensor(gt_flows[idx], dtype=torch.float32, device=device).reshape(H, W, 2)
                    ok = torch.isfinite(gt).all(-1)
                    if flow_valid is not None:
                        ok = ok & (torch.as_tensor(flow_valid[idx], device=device).reshape(H, W) != 0)
                    err = torch.linalg.vector_norm(flows[-1] - torch.where(ok[..., None], gt, torch.zeros_like(gt)), dim=-1)
                    epes.append(torch.where(ok, err, torch.zeros_like(err)).sum() / ok.sum())
            if gt_depths is not None:
                dlosses.append(compute_depth_loss(res[1], torch.as_tensor(gt_depths[idx], dtype=torch.float32, device=device), skip_holes=True))
            if with_distortion:
                wts = res[3].reshape(H * W, -1)
                d_loss, _, d_map = distortion_loss_raw(wts, delta, out=(torch.empty((), device=wts.device), None, torch.empty(H * W, device=wts.device)))
                dists.append(d_loss)
                dmaps.append(d_map.reshape(H, W))
            rgb = rgb.reshape(H, W, 3)
            if targets is not None:
                tgt = torch.as_tensor(targets[idx], dtype=torch.float32, device=device).reshape(H, W, 3)
                psnrs.append(mse2psnr(float(torch.mean((rgb - tgt) ** 2))))
                if with_ssim:
                    ssims.append(ssim_frames(rgb, tgt))
            imgs.append((rgb.clamp(0, 1).cpu().numpy() * 255.0).astype(np.uint8))
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        try:
            from PIL import Image
            for idx, img in enumerate(imgs):
                Image.fromarray(img).save(os.path.join(savedir, "r_%03d.png" % idx))
            if flows:
                from .flow_vis import flow_to_rgb
                for idx, fl in enumerate(flows):
                    Image.fromarray((flow_to_rgb(fl).cpu().numpy() * 255.0).astype(np.uint8)).save(os.path.join(savedir, "r_%03d_flow.png" % idx))
        except ImportError:      # no image writer in this environment: keep the raw frames
            np.save(os.path.join(savedir, "frames.npy"), np.stack(imgs))
    out = {"psnr": psnrs, "mean_psnr": (sum(psnrs) / len(psnrs)) if psnrs else None, "images": np.stack(imgs)}
    if flows:
        out["flow2d"] = torch.stack(flows).cpu().numpy()
    if with_ssim:
        out["ssim"] = torch.cat(ssims).cpu().tolist() if ssims else []
        out["mean_ssim"] = (sum(out["ssim"]) / len(out["ssim"])) if ssims else None
    if gt_depths is not None:
        out["depth_loss"] = torch.stack(dlosses).cpu().tolist() if dlosses else []
        out["mean_depth_loss"] = (sum(out["depth_loss"]) / len(out["depth_loss"])) if dlosses else None
    if gt_flows is not None:
        out["epe"] = torch.stack(epes).cpu().tolist() if epes else []
        out["mean_epe"] = (sum(out["epe"]) / len(out["epe"])) if epes else None
    if with_distortion:
        out["distortion"] = torch.stack(dists).cpu().tolist() if dists else []
        out["mean_distortion"] = (sum(out["distortion"]) / len(out["distortion"])) if dists else None
        out["distortion_maps"] = torch.stack(dmaps).cpu().numpy() if dmaps else np.zeros((0, H, W), np.float32)
    return out


def _save_layers(savedir, idx, obj_rgb, obj_acc):
    """r_%03d_obj%d.png: one straight-alpha RGBA image per object of frame idx (raw arrays where no image writer is installed)"""
    import numpy as np
    from .objects_vis import layer_to_rgba
    os.makedirs(savedir, exist_ok=True)
    for k in range(obj_acc.shape[-1]):
        img = (layer_to_rgba(obj_rgb, obj_acc, k).cpu().numpy() * 255.0).astype(np.uint8)
        try:
            from PIL import Image
            Image.fromarray(img, "RGBA").save(os.path.join(savedir, "r_%03d_obj%d.png" % (idx, k)))
        except ImportError:
            np.save(os.path.join(savedir, "r_%03d_obj%d.npy" % (idx, k)), img)


def render_segm_evaluation(nvfi, renderer, mask_field, poses, times, gt_segms, H, W, focal, near, far, white_background=True,
                           savedir=None, ignore_npoint_thresh=0, n_gt=None, device=None, return_maps=False, with_layers=False):
    """The loop of the reference's test_segm_render.py:87-180 on this path: with `mask_field` attached to the field, one
    `Renderer.render(mode='test', transfer_vel=True)` per (pose, time) frame, whose composited mask map (H,W,K) goes straight into
    utils.metric_segm.SegmEvaluator together with the frame's ground-truth labels `gt_segms[i]` (H,W; integers in [0, 32), 0 the background):
    the kernel call is queued behind the frame and nothing waits for the device until the summary brings the per-frame matrices over.
    `savedir`: r_%03d_segm_vis.png per frame - the predicted labels aligned to the ground truth's object order (point_segm_util.align_insts'
    rule), as 8-bit grey levels (the reference's colour table is not part of this project).

    Returns SegmEvaluator.summary(): {"AP", "PQ", "F1", "Pre", "Rec", "mIoU", "RI", ...}; return_maps=True adds "segm_maps", the rendered mask
    maps (device tensors).  with_layers=True (default off: the function is as before) renders every frame through Renderer.render_objects
    instead - same mask map - and, with `savedir`, writes each object's layer as a straight-alpha RGBA image r_%03d_obj%d.png
    (utils.objects_vis.layer_to_rgba)."""
    import numpy as np
    from ..models import Camera
    from .metric_segm import SegmEvaluator
    device = device or next(nvfi.parameters()).device
    field = nvfi.nvfi
    saved, field.mask_field = field.mask_field, mask_field
    nvfi.eval()
    ev, maps = None, []
    try:
        with torch.no_grad():
            for idx in range(len(poses)):
                pose = torch.as_tensor(poses[idx], dtype=torch.float32, device=device)
                cam = Camera(pose, H, W, focal, None, near, far)
                if with_layers:
                    res = renderer.render_objects(float(times[idx]), cam.rays.to(device), white_background=white_background, transfer_vel=True)
                    segm_map = res[4]
                    if savedir is not None:
                        _save_layers(savedir, idx, res[5].reshape(H, W, -1, 3), res[6].reshape(H, W, -1))
                else:
                    segm_map = renderer.render(float(times[idx]), cam.rays.to(device), white_background=white_background, mode="test", transfer_vel=True)[4]
                segm_map = segm_map.reshape(H, W, -1)
                if ev is None:
                    ev = SegmEvaluator(segm_map.shape[-1], n_gt, keep_labels=savedir is not None)
                ev.update(segm_map, torch.as_tensor(gt_segms[idx], device=device).reshape(H, W))
                if return_maps:
                    maps.append(segm_map)
    finally:
        field.mask_field = saved
    out = ev.summary(ignore_npoint_thresh, aligned=savedir is not None)
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        labels = torch.stack(out["aligned"]).cpu().numpy()
        vis = (labels * (255 // max(int(labels.max()), 1))).astype(np.uint8)
        try:
            from PIL import Image
            for idx, img in enumerate(vis):
                Image.fromarray(img).save(os.path.join(savedir, "r_%03d_segm_vis.png" % idx))
        except ImportError:      # no image writer in this environment: keep the raw label maps
            np.save(os.path.join(savedir, "segm_labels.npy"), labels)
    if return_maps:
        out["segm_maps"] = maps
    return out
