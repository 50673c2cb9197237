"""Colour coding of an optical-flow map: hue from the direction, saturation from the magnitude (the usual HSV flow wheel), in torch ops."""
import math

import torch


def flow_to_rgb(flow_hw2, max_mag=None):
    """flow (..., 2) = (u, v) in pixels, u to the right and v DOWN the image -> rgb (..., 3) in [0, 1] on the flow's device.

    hue = atan2(v, u) / 2 pi (u > 0: red, v > 0: yellow-green at 90 degrees, u < 0: cyan, v < 0: blue-violet at 270 degrees), saturation =
    min(|flow| / max_mag, 1), value 1: no motion is white.  max_mag None: the largest magnitude of the map (1 for an all-zero map)."""
    f = torch.as_tensor(flow_hw2, dtype=torch.float32)
    u, v = f[..., 0], f[..., 1]
    mag = torch.sqrt(u * u + v * v)
    if max_mag is None:
        m = mag.max() if mag.numel() else mag.new_tensor(0.0)
        max_mag = torch.where(m > 0, m, torch.ones_like(m))
    sat = (mag / max_mag).clamp(0.0, 1.0)
    hue = torch.remainder(torch.atan2(v, u) / (2.0 * math.pi), 1.0)
    # HSV -> RGB with value 1: channel = 1 - sat * (1 - clamp(|6 h - c| - 1, 0, 1)) for the three phase-shifted triangle waves
    h6 = hue * 6.0
    r = (torch.abs(h6 - 3.0) - 1.0).clamp(0.0, 1.0)
    g = (2.0 - torch.abs(h6 - 2.0)).clamp(0.0, 1.0)
    b = (2.0 - torch.abs(h6 - 4.0)).clamp(0.0, 1.0)
    rgb = torch.stack([r, g, b], dim=-1)
    return 1.0 - sat[..., None] * (1.0 - rgb)
