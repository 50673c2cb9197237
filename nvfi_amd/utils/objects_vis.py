"""Per-object layers of Renderer.render_objects as images, in torch ops: a layer as straight-alpha RGBA, the cheap 2-D recombination of
finished layers, and the hard label map."""
import torch


def layer_to_rgba(obj_rgb, obj_acc, k, eps=1e-6):
    """layer k of obj_rgb (..., K, 3) (premultiplied: sum w m_k c) and obj_acc (..., K) (sum w m_k) -> (..., 4) straight-alpha RGBA in [0, 1]:
    colour = obj_rgb / obj_acc where obj_acc > eps (0 elsewhere: a guarded divide), alpha = obj_acc."""
    c = torch.as_tensor(obj_rgb, dtype=torch.float32)[..., k, :]
    a = torch.as_tensor(obj_acc, dtype=torch.float32)[..., k]
    ok = a > eps
    col = torch.where(ok[..., None], c / torch.where(ok, a, torch.ones_like(a))[..., None], torch.zeros_like(c))
    return torch.cat([col.clamp(0.0, 1.0), a.clamp(0.0, 1.0)[..., None]], -1)


def composite_layers(obj_rgb, obj_acc, keep, white_background=True):
    """The 2-D recombination of finished layers: rgb (..., 3) = sum_{k in keep} obj_rgb_k (+ 1 - sum_{k in keep} obj_acc_k on a white background),
    clamped to [0, 1].  `keep`: object indices, or K factors in [0, 1] (floating point).

    NOT occlusion-correct: every layer was composited behind whatever stood in front of it in the render it came from, so dropping the object in
    front leaves a hole (or the background), not the surface behind it.  Renderer.render_objects(select=...) re-renders the scene with the density
    of the removed objects gone and recomputes the transmittance: use that when occlusion matters, this when a quick preview will do."""
    c = torch.as_tensor(obj_rgb, dtype=torch.float32)
    a = torch.as_tensor(obj_acc, dtype=torch.float32).to(c.device)
    K = a.shape[-1]
    kp = torch.as_tensor(keep)
    if kp.dtype.is_floating_point:
        f = kp.reshape(-1).to(device=c.device, dtype=torch.float32)
        if f.numel() != K:
            raise ValueError(f"keep: {f.numel()} factors for {K} layers")
    else:
        f = torch.zeros(K, dtype=torch.float32, device=c.device)
        f[kp.reshape(-1).long().to(c.device)] = 1.0
    rgb = (c * f[:, None]).sum(-2)
    if white_background:
        rgb = rgb + (1.0 - (a * f).sum(-1))[..., None]
    return rgb.clamp(0.0, 1.0)


def label_map(obj_acc, min_acc=0.0):
    """hard labels (...,) int64: argmax_k obj_acc; -1 where the ray's total opacity sum_k obj_acc is <= min_acc (nothing was hit)"""
    a = torch.as_tensor(obj_acc, dtype=torch.float32)
    lab = a.argmax(-1)
    return torch.where(a.sum(-1) > min_acc, lab, torch.full_like(lab, -1))
