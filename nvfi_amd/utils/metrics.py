"""Image metrics of the reference's evaluation (utils/metrics.py; train_nvfi.py --eval_test prints them per test set) with its names and
signatures: `from utils.metrics import SSIM, estim_error` becomes `from nvfi_amd.utils.metrics import ...`.

SSIM runs on the kernel nvfi_ssim (csrc/metrics.hip): the images are read in place through their strides - the reference's (B, C, H, W) and the
renderer's own (H, W, 3) frames (`ssim_frames`) alike, no permute copy - the dynamic range is derived on the device by the reference's rule, and
nothing is brought to the host: the result is a device tensor, as the reference's is.  There is no CPU path: CPU tensors raise NvfiError.
MSE / PSNR are the reference's two torch expressions.  LPIPS needs the `lpips` package and its VGG weights; `estim_error` reports it only when
that package can be imported, and never fetches anything.

Differences from the reference: `w_size` other than 11 raises NotImplementedError; the window moments are accumulated in fp64 (the reference:
fp32 conv2d), so the value is the float64 one to about 1e-8; `estim_error` returns plain floats."""
import ctypes as C
import math
import os

import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr


def mse2psnr(mse):
    """utils/metrics.py:11-15 of the reference."""
    if mse == 0:
        mse = 1e-5
    return -10.0 * math.log10(mse)


class MSE(object):
    def __call__(self, pred, gt):
        return torch.mean((pred - gt) ** 2)


class PSNR(object):
    def __call__(self, pred, gt):
        mse = torch.mean((pred - gt) ** 2)
        return 10 * torch.log10(1 / mse)


def ssim_stats(pred, gt, layout="BCHW", L=None, per_image_range=False):
    """(B, 2) float64 device tensor: per image the mean of the SSIM map and the mean of cs = v1 / v2 (metrics.py:86-90).  `layout` names the axes
    of the 4-d inputs ("BCHW" or "BHWC"); L = None derives the dynamic range from `pred` on the device (over the whole call, or per image)."""
    if not (pred.is_cuda and gt.is_cuda):
        raise _lib.NvfiError("SSIM runs on the GPU only (no CPU fallback exists)")
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"SSIM expects two 4-d tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if layout not in ("BCHW", "BHWC"):
        raise ValueError("layout must be 'BCHW' or 'BHWC'")
    pred, gt = pred.detach(), gt.detach()
    if pred.dtype != torch.float32:
        pred = pred.float()
    if gt.dtype != torch.float32:
        gt = gt.float()
    order = (0, 1, 2, 3) if layout == "BCHW" else (0, 3, 1, 2)      # positions of (image, channel, row, column)
    B, Cc, H, W = (pred.shape[i] for i in order)
    if not 1 <= Cc <= 4:
        raise NotImplementedError("1..4 channels are supported")
    if H < 11 or W < 11:
        raise ValueError("the 11 x 11 window has no padding: images must be at least 11 x 11")
    if any(s < 0 for s in pred.stride() + gt.stride()):
        pred, gt = pred.contiguous(), gt.contiguous()
    ps = (C.c_int64 * 4)(*[pred.stride(i) for i in order])
    gs = (C.c_int64 * 4)(*[gt.stride(i) for i in order])
    win = (C.c_float * 11)(*SSIM().gaussian(11, 1.5).tolist())
    out = torch.empty(B, 2, dtype=torch.float64, device=pred.device)
    lib = _lib.lib()
    nbytes = _lib.bytes_of(lib.nvfi_metrics_workspace_bytes, 0, B, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    mode = 0 if L is not None else (2 if per_image_range else 1)
    with torch.cuda.device(pred.device):
        _lib.check(lib.nvfi_ssim(B, Cc, H, W, _lib.ptr(pred), ps, _lib.ptr(gt), gs, win, float(L or 0.0), mode, _lib.ptr(out),
                                 _lib.ptr(ws), ws.numel(), _stream_ptr()))
    return out


class SSIM(object):
    """structural similarity index (utils/metrics.py:32-99): 11-tap Gaussian window (sigma 1.5), no padding, per channel"""

    def gaussian(self, w_size, sigma):
        gauss = torch.Tensor([math.exp(-(x - w_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(w_size)])
        return gauss / gauss.sum()

    def create_window(self, w_size, channel=1):
        w = self.gaussian(w_size, 1.5).unsqueeze(1)
        return w.mm(w.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, w_size, w_size).contiguous()

    def __call__(self, y_pred, y_true, w_size=11, size_average=True, full=False):
        """y_pred, y_true (B, C, H, W) on the GPU -> SSIM (larger is better): a 0-d tensor, or (B,) with size_average=False; with full=True also
        cs, the mean of v1 / v2 over the whole batch"""
        if w_size != 11:
            raise NotImplementedError("the kernel is written for the 11-tap window")
        st = ssim_stats(y_pred, y_true, "BCHW")
        ret = (st[:, 0].mean() if size_average else st[:, 0]).float()
        if full:
            return ret, st[:, 1].mean().float()
        return ret


def ssim_frames(pred_hwc, gt_hwc):
    """SSIM of channel-last frames as the renderer returns them - (H, W, C) or (B, H, W, C) - read in place; the dynamic range is derived per
    frame, which is what the reference's frame-by-frame loop does (metrics.py:149).  Returns a (B,) float64 device tensor."""
    if pred_hwc.dim() == 3:
        pred_hwc, gt_hwc = pred_hwc[None], gt_hwc[None]
    return ssim_stats(pred_hwc, gt_hwc, "BHWC", per_image_range=True)[:, 0]


@torch.no_grad()
def estim_error(estim, gt):
    """estim, gt (B, C, H, W) in [0, 1] on the GPU -> {"mse", "psnr", "ssim"} (+ "lpips" when the lpips package is importable), as
    utils/metrics.py:141-152: SSIM is the mean of the per-image values, each with its own derived dynamic range"""
    errors = dict()
    errors["mse"] = MSE()(estim, gt).item()
    errors["psnr"] = PSNR()(estim, gt).item()
    errors["ssim"] = float(ssim_stats(estim, gt, "BCHW", per_image_range=True)[:, 0].mean().item())
    try:
        import lpips
    except ImportError:
        lpips = None
    # lpips.LPIPS(net="vgg") loads torchvision's VGG-16 checkpoint and would fetch it when it is not in the hub cache: only with the file present
    vgg = os.path.join(torch.hub.get_dir(), "checkpoints", "vgg16-397923af.pth")
    if lpips is not None and os.path.exists(vgg):
        model = lpips.LPIPS(net="vgg").eval().to(estim.device)
        errors["lpips"] = float(sum(torch.mean(model.forward(estim[i:i + 1] * 2.0 - 1.0, gt[i:i + 1] * 2.0 - 1.0)).item()
                                    for i in range(estim.shape[0])) / estim.shape[0])
    return errors


def save_error(errors, save_dir, ext=''):
    save_path = os.path.join(save_dir, f"metrics{ext}.txt")
    with open(save_path, "w") as f:
        f.write(str(errors))
