"""Helper of tests/test_gpu_flowloss.py (run in a subprocess with NVFI_DETERMINISTIC=1, which is read once per process and makes the plane
scatter and the weight-gradient reduce bit-reproducible): the gradient comparisons of the flow term that need bit-reproducible render gradients.
Writes every gradient to the .npz named on the command line and prints one JSON line:

  plain_repeats   two plain render + mse backwards give the same bits per tensor (the mode is on)
  untouched       per tensor outside weight_net: the backward of mse + 0.5 flow_loss(weight_grad=False) gives the bits of the plain backward
  ws_same         the render workspace has the same bytes before and after the flow call
  net_moved       the flow term reaches every weight_net tensor

.npz: "ref:<name>" the gradients of SCALE * (mse + LAM * flow_loss) through autograd, "got:<name>" those of the fused driver
render_mse_backward_(loss_scale=SCALE, flow_weight=LAM, target_flow=...), "weights" the render's weights, "flow" the two loss values."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_flowloss as tg                   # noqa: E402
from conftest import GOLD                        # noqa: E402

LAM, SCALE = 0.5, 0.25                           # powers of two: scaling g_weights on the host or inside the kernel rounds alike


def main(out_path):
    c = tg._make_ctx(np.load(os.path.join(GOLD, "hotpath.npz")), "A")["A"]
    model, f = c["model"], c["f"]
    o, d, jit, target, valid = tg._case(c, "A", 65)
    dt = tg._dt(c, 1)
    rgb_t = tg._cu(np.random.default_rng(3).random((65, 3)))
    tgt, val = tg._cu(target), tg._cu(valid, np.uint8)
    ws_same = []

    def run(flow):
        model.zero_grad(set_to_none=True)
        out = tg._render(c, o, d, jit)
        loss = torch.nn.functional.mse_loss(out[0], rgb_t)
        if flow:
            ws = out[3].grad_fn.ws
            before = ws.clone()
            loss = loss + 0.5 * f.flow_loss(out[3], dt, c["cam"], tgt, valid=val, weight_grad=False)
            ws_same.append(bool(torch.equal(ws, before)))
        loss.backward()
        return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}

    p1, p2, fl = run(False), run(False), run(True)
    own = [k for k, g in p1.items() if g is not None and not tg._is_weight_net(k)]
    net = [k for k, g in p1.items() if g is not None and tg._is_weight_net(k)]
    res = dict(plain_repeats={k: bool(torch.equal(p1[k], p2[k])) for k in own + net},
               untouched={k: bool(fl[k] is not None and torch.equal(fl[k], p1[k])) for k in own},
               none_stay_none=all(fl[k] is None for k, g in p1.items() if g is None),
               ws_same=bool(ws_same and all(ws_same)), net_moved={k: not torch.equal(fl[k], p1[k]) for k in net})

    # the two forms of the whole step
    model.zero_grad(set_to_none=True)
    out = tg._render(c, o, d, jit)
    flow = f.flow_loss(out[3], dt, c["cam"], tgt, valid=val)
    (SCALE * (torch.nn.functional.mse_loss(out[0], rgb_t) + LAM * flow)).backward()
    save = {"weights": out[3].detach().cpu().numpy()}
    for k, p in model.named_parameters():
        if p.grad is not None:
            save["ref:" + k] = p.grad.detach().cpu().numpy().copy()
    cam_dev = (tg._cu(c["cam"][0]),) + tuple(c["cam"][1:])
    r = tg._fused(c, o, d, jit, rgb_t, loss_scale=SCALE, target_flow=tgt, flow_dt=dt, flow_camera=cam_dev, flow_weight=LAM, flow_valid=val)
    for k, p in model.named_parameters():
        if "ref:" + k in save:
            save["got:" + k] = p.grad.detach().cpu().numpy().copy()
    save["flow"] = np.array([float(flow.detach()), float(r[2])], np.float64)
    np.savez(out_path, **save)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
