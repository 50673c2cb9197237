"""Helper of tests/test_gpu_maskloss.py (run in a subprocess with NVFI_DETERMINISTIC=1, which is read once per process and makes the plane
scatter and the weight-gradient reduce bit-reproducible): the two forms of the whole training step with a mask term.  Writes every gradient to
the .npz named on the command line:

  "ref:<name>" the gradients of SCALE * (mse + LAM * mask_loss) through autograd, "got:<name>" those of the fused driver
  render_mse_backward_(loss_scale=SCALE, mask_weight=LAM, target_mask=...); the MaskField's ten tensors under "mask:<key>";
  "weights" the render's weights, "loss" the two mask-loss values."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import maskloss64 as ml64                        # noqa: E402
import test_gpu_maskloss as tg                   # noqa: E402
from conftest import GOLD                        # noqa: E402

LAM, SCALE = 0.5, 0.25                           # powers of two: scaling g_weights on the host or inside the kernel rounds alike


def main(out_path):
    c = tg._make_ctx(np.load(os.path.join(GOLD, "hotpath.npz")), "A")["A"]
    model, f = c["model"], c["f"]
    K, R = 8, 33
    mf = c["mfs"][K]
    o, d, jit = tg._rays(c, R)
    rgb_t = tg._cu(np.random.default_rng(3).random((R, 3)))
    tgt = tg._cu(tg._target(R, K, False), np.int32)
    model.zero_grad(set_to_none=True)
    mf.zero_grad(set_to_none=True)
    out = tg._render(c, o, d, jit)
    ml = f.mask_loss(out[3], tgt, mask_field=mf, kind="ce", eps=tg.EPS)
    (SCALE * (torch.nn.functional.mse_loss(out[0], rgb_t) + LAM * ml)).backward()
    save = {"weights": out[3].detach().cpu().numpy()}
    for k, p in model.named_parameters():
        if p.grad is not None:
            save["ref:" + k] = p.grad.detach().cpu().numpy().copy()
    for k, p in zip(ml64.GRAD_KEYS, mf._params()):
        save["ref:mask:" + k] = p.grad.detach().cpu().numpy().copy()
    r = tg._fused(c, K, o, d, jit, rgb_t, loss_scale=SCALE, target_mask=tgt, mask_weight=LAM, mask_eps=tg.EPS)
    for k, p in model.named_parameters():
        if "ref:" + k in save:
            save["got:" + k] = p.grad.detach().cpu().numpy().copy()
    for k, p in zip(ml64.GRAD_KEYS, mf._params()):
        save["got:mask:" + k] = p.grad.detach().cpu().numpy().copy()
    save["loss"] = np.array([float(ml.detach()), float(r[2])], np.float64)
    np.savez(out_path, **save)


if __name__ == "__main__":
    main(sys.argv[1])
