#!/usr/bin/env python
"""Golden vectors of the depth loss (nvfi_depth_loss), generated from the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_depth.py        (reference checkout as in make_golden.py)
Writes tests/golden/depthloss.npz (numbers only).

Unit cases `<case>:<n>:{pred,gt,loss,grad}`: the reference's own compute_depth_loss (utils/evaluation_utils.py:8-17) in fp32 with its autograd
gradient, n in {1, 2, 3, 64, 65, 2048}, for the named cases of depth64.named_case: distinct | plateau (60 % of pred equal to far: the median
lies in the ties) | allequal | signed (negative values, -0.0 and +0.0 among the entries).
  ref32_err:loss    largest absolute error of the reference's fp32 loss against depth64 (float64) over the unit cases
  ref32_err:grad    largest error of its gradient relative to depth64.grad_scale: max|grad| of the yardstick, or - on the cases where the
                    gradient is a cancellation of more than 10 bits of its own terms (n = 2: the normalised map is (0, 2) whatever the depths
                    are, the exact gradient is ~0) - the size of those terms (the distance of the fp32 reference from exact arithmetic:
                    what bounds the GPU test)
  ref32_err:grad_raw  the same with max|grad| on every case: 1.2e-2, set by the two ill-conditioned n = 2 cases alone (documentation; no
                    test uses it)

End-to-end case `e2e:*`: the reference's training render of golden field A with rays, jitter (torch.manual_seed(21)) and colour target of
hotpath.npz's A:train_nonkey, loss = mse(rgb, target) + w * compute_depth_loss(depth[subset], gt[subset]).  gt is seeded uniform in
[near, far], unrelated to the rendered depth, so u - v is O(1) and the gradient is not a difference of near-equal numbers.  Stored: t, w,
depth, gt (0 = hole at every ray outside the subset), subset, loss_mse, loss_depth, g_depth, g_rgb, grad:<parameter> for every parameter
whose name does not contain one of E2E_SKIP: the tensors that receive no gradient from the depth map (depth is a sum of weights x distances:
app_plane_space.*, the render MLP's two large weight matrices - their g_rgb path is pinned by hotpath.npz's train_nonkey case on the same rays) and four of the
velocity net's four hidden 128 x 128 weight matrices drop three (60 KB each; the first layer, one hidden matrix, the last layer and every
bias stay).
ASSERTS: the render reproduces hotpath.npz's depth; the reference's median depth keeps at least 10 x the depth contract of
helpers.assert_contract (rtol 1e-4 + its fp32 floor) from both neighbours in sorted order - rays are dropped from the subset until it does,
otherwise a last-bit difference of the render could hand the median to another ray and its gradient to another place."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import depth64 as d64  # noqa: E402

SIZES = (1, 2, 3, 64, 65, 2048)
CASES = ("distinct", "plateau", "allequal", "signed")
W_DEPTH = 0.1
MIN_SUBSET = 64
E2E_SKIP = ("app_plane_space", "renderModule.mlp.0.weight", "renderModule.mlp.2.weight", "vel_net.weight_net.4.0.weight",
            "vel_net.weight_net.5.0.weight", "vel_net.weight_net.6.0.weight")


def case_seed(ci, n):
    return 1000 * (ci + 1) + n


def reference_loss(fn, pred, gt):
    p = torch.from_numpy(pred.copy()).requires_grad_(True)
    loss = fn(p, torch.from_numpy(gt.copy()))
    loss.backward()
    return np.float32(loss.item()), mg.npf(p.grad)


def median_margin(depth, subset):
    """(gap of the median of depth[subset] to its nearer neighbour in sorted order, required gap, subset position of that neighbour)"""
    d = depth[subset].astype(np.float64)
    order = np.argsort(d, kind="stable")
    k = (len(d) - 1) // 2
    need = 10 * (1e-4 * abs(d[order[k]]) + 2e-5)
    gaps = [(abs(d[order[j]] - d[order[k]]), int(order[j])) for j in (k - 1, k + 1) if 0 <= j < len(d)]
    gap, who = min(gaps)
    return gap, need, who


def main():
    R = mg.import_reference()
    from utils.evaluation_utils import compute_depth_loss as ref_fn
    torch.set_num_threads(4)
    fx = {}
    worst = {"loss": 0.0, "grad": 0.0, "grad_raw": 0.0}
    ill = []
    for ci, case in enumerate(CASES):
        for n in SIZES:
            pred, gt = d64.named_case(case, n, case_seed(ci, n))
            loss, grad = reference_loss(ref_fn, pred, gt)
            y = d64.depth64(pred, gt)
            e_loss, e_grad = d64.errors(loss, grad, y)
            worst["loss"], worst["grad"] = max(worst["loss"], e_loss), max(worst["grad"], e_grad)
            worst["grad_raw"] = max(worst["grad_raw"], d64.error_vs_gmax(grad, y))
            if d64.grad_scale(y) != np.abs(y["grad"]).max():
                ill.append(f"{case}:{n}")
            key = f"{case}:{n}"
            fx[key + ":pred"], fx[key + ":gt"], fx[key + ":loss"], fx[key + ":grad"] = pred, gt, loss, grad
            ties = int((pred == np.float32(y["med_pred"])).sum())
            print(f"{key}: loss {float(loss):.6e} (yardstick {y['loss']:.6e}, err {e_loss:.1e}) grad err {e_grad:.1e} of max {np.abs(y['grad']).max():.3e}, "
                  f"median {y['med_pred']:.6g} x{ties}")
            if case == "plateau" and n >= 3:
                assert ties >= n // 2 and y["med_pred"] == 8.0
            if case == "signed":
                assert np.signbit(pred[pred == 0]).any() and (n == 1 or (~np.signbit(pred[pred == 0])).any())
            if n == 1:
                assert float(loss) == 0.0 and not grad.any() and y["loss"] == 0.0 and not y["grad"].any()
    fx["ref32_err:loss"], fx["ref32_err:grad"] = np.float64(worst["loss"]), np.float64(worst["grad"])
    fx["ref32_err:grad_raw"] = np.float64(worst["grad_raw"])
    print("ref32_err:", worst, "ill-conditioned gradients (measured against the size of their terms):", ill)
    assert all(k.endswith(":2") for k in ill), ill

    # ---- end to end on field A
    hot = np.load(os.path.join(HERE, "hotpath.npz"))
    cfgA, nvA = mg.build_field(R, "A")
    ren = R["Renderer"](nvA, 0, 0, 2048)
    o, d = torch.from_numpy(hot["A:rays_o"]), torch.from_numpy(hot["A:rays_d"])
    tt = float(hot["A:train_nonkey:t"])
    target = torch.from_numpy(hot["A:train_nonkey:target"])
    nvA.zero_grad(set_to_none=True)
    torch.manual_seed(21)
    out = ren.render(tt, R["Ray"](o, d, 0, 1), white_background=cfgA.dataset.white_background, mode="train")
    rgb, depth = out[0], out[1]
    assert np.array_equal(mg.npf(depth), hot["A:train_nonkey:depth"]) and np.array_equal(mg.npf(rgb), hot["A:train_nonkey:rgb"])
    rgb.retain_grad()
    depth.retain_grad()
    near, far = float(nvA.nvfi.near_far[0]), float(nvA.nvfi.near_far[1])
    nR = depth.shape[0]
    gt = np.random.default_rng(4242).uniform(near, far, nR).astype(np.float32)
    dnp = mg.npf(depth).reshape(-1)
    subset = np.arange(nR)
    while True:
        gap, need, who = median_margin(dnp, subset)
        if gap >= need:
            break
        subset = np.delete(subset, who)
        assert len(subset) >= MIN_SUBSET, "the median of the rendered depth cannot be isolated"
    print(f"e2e: {len(subset)} of {nR} rays, median gap {gap:.3e} >= {need:.3e}")
    sub = torch.from_numpy(subset)
    loss_mse = torch.nn.functional.mse_loss(rgb, target)
    loss_depth = ref_fn(depth.reshape(-1)[sub], torch.from_numpy(gt)[sub])
    (loss_mse + W_DEPTH * loss_depth).backward()
    gt_holes = np.zeros(nR, np.float32)
    gt_holes[subset] = gt[subset]
    y = d64.depth64(dnp, gt_holes, skip_holes=True)
    e_loss, e_grad = d64.errors(float(loss_depth), mg.npf(depth.grad).reshape(-1) / W_DEPTH, y)
    print(f"e2e: mse {float(loss_mse):.6e} depth loss {float(loss_depth):.6e} (yardstick {y['loss']:.6e}, err {e_loss:.1e}, grad err {e_grad:.1e})")
    assert y["n_counted"] == len(subset) and e_loss <= 4 * max(worst["loss"], 2.0 ** -23 * y["loss"]) and e_grad <= 4 * max(worst["grad"], 2.0 ** -23)
    fx["e2e:t"], fx["e2e:w"] = np.float64(tt), np.float64(W_DEPTH)
    fx["e2e:depth"], fx["e2e:gt"], fx["e2e:subset"] = dnp, gt_holes, subset.astype(np.int64)
    fx["e2e:loss_mse"], fx["e2e:loss_depth"] = np.float32(loss_mse.item()), np.float32(loss_depth.item())
    fx["e2e:g_depth"], fx["e2e:g_rgb"] = mg.npf(depth.grad).reshape(-1), mg.npf(rgb.grad)
    for k, p in nvA.named_parameters():
        if k.startswith("nvfi.vel.vel_net.") or any(w in k for w in E2E_SKIP):
            continue
        fx[f"e2e:grad:{k}"] = mg.npf(p.grad) if p.grad is not None else np.zeros(0, np.float32)
    path = os.path.join(HERE, "depthloss.npz")
    np.savez_compressed(path, **fx)
    print("wrote depthloss.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400000


if __name__ == "__main__":
    main()
