#!/usr/bin/env python
"""Optical-flow supervision of a training render (field.flow_loss / render_mse_backward_(target_flow=): nvfi_flow_loss_fwd + nvfi_flow_loss_bwd;
csrc/flowloss.hip) on the bench's bat scene (bench.build_scene: 199^3 grid, K = 16), 2 048 rays x 128 samples, one and four RK2 steps, timed on
the GPU behind ONE training render that stays alive (the term's own cost, not the render's):
  raw forward            nvfi_flow_loss_fwd: gather, no-grad warp, per-ray map + loss terms, mean, g_weights + g_xd
  raw forward + backward + the chunked nvfi_flow_loss_bwd (pack, stash-writing warp, unfused adjoint, weight-gradient jobs) into kept gradient buffers:
                         what the fused driver adds to a step
  autograd form          field.flow_loss(...) + torch.autograd.grad to the 12 tensors of weight_net (weight_grad off: the render's backward is not
                         part of the term)
  torch form             the same loss assembled by hand: mask = weights > thres, the sample depths rebuilt from the jitter and the t_min rule,
                         field.advect on the masked positions, projection, index_add, and autograd to weights and weight_net
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds; the masked count, workspace bytes and chunk count are printed.
    python tools/bench_flowloss.py [--out profiles/flowloss_timing.txt] [--max-workspace-bytes B]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def torch_form(f, o, d, u, weights, t, dt, pose, focal, target):
    """the hand-assembled term: -> loss, with autograd to `weights` (a leaf) and to weight_net through field.advect"""
    aabb, S = f.aabb, weights.shape[1]
    near, far = float(f.near_far[0]), float(f.near_far[1])
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    if bool(((aabb[0] <= o) & (o <= aabb[1])).any()):
        t_min = torch.full_like(o[:, 0], near)
    else:
        t_min = torch.minimum((aabb[1] - o) / vec, (aabb[0] - o) / vec).amax(-1).clamp(min=near, max=far)
    z = t_min[:, None] + float(f._step_host) * (torch.arange(S, device=o.device)[None].float() + u[:, None])
    mask = weights.detach() > f.rayMarch_weight_thres
    idx = mask.nonzero()
    ray = idx[:, 0]
    zm = z[mask]
    half = (aabb[1] - aabb[0]) / 2
    x = (o[ray] + d[ray] * zm[:, None] - aabb[0]) / half - 1
    xd = f.advect(x, t, t + dt)

    def pix(xn):
        c = (aabb[0] + (xn + 1) * half - pose[:, 3]) @ pose[:, :3]
        return torch.stack([focal * c[:, 0] / -c[:, 2], -(focal * c[:, 1] / -c[:, 2])], 1), -c[:, 2]

    p0, _ = pix(x)
    p1, z1 = pix(xd)
    d2 = torch.where((z1.detach() < 1e-3)[:, None], torch.zeros_like(p0), p1 - p0)
    flow2d = torch.zeros(o.shape[0], 2, device=o.device).index_add(0, ray, weights[mask][:, None] * d2)
    return torch.nn.functional.mse_loss(flow2d, target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-workspace-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flowloss needs the GPU: there is no CPU fallback"
    import bench
    from nvfi_amd.utils import flow_loss as fl
    model = bench.build_scene("cuda")
    f = model.nvfi
    K, R = int(f.num_keyframes), a.rays
    ts = float(f.tmax) / (K - 1)
    bo, bd = bench.camera_bundle("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    sel = torch.randperm(bo.shape[0], device="cuda", generator=g)[:R]
    o, d = bo[sel].contiguous(), bd[sel].contiguous()
    u = torch.rand(R, device="cuda", generator=g)
    pose = bench.pose_spherical(30.0, -30.0, 4.0)[:3, :4].contiguous().cuda()
    focal = float(np.float32(0.5 * bench.W_IMG / np.tan(0.5 * bench.ANGLE_X)))
    cam = (pose, bench.H_IMG, bench.W_IMG, focal)
    target = torch.randn(R, 2, device="cuda", generator=g)
    t = 1.25 * ts
    params = list(f._render_params()[19:31])
    model.train()
    f.jitter_override = u.reshape(-1, 1).cpu()
    try:
        out = f(t, o, d, True)
    finally:
        f.jitter_override = None
    weights = out[3]
    node = weights.grad_fn
    ro, rd, w = node.saved_tensors[:3]
    M = int(f.last_counters[2])
    desc = f._desc()
    grads = [torch.zeros_like(p) for p in params]
    G = f._grads_struct_vel(grads + [None] * 12)
    wl = w.detach().clone().requires_grad_(True)
    lines = [f"flow loss behind one training render, R = {R} rays x {w.shape[1]} samples, {M} masked samples, bat scene {f.gridSize.tolist()} K = {K}; "
             f"{torch.cuda.get_device_name(0)}; max_workspace_bytes = {a.max_workspace_bytes}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max], us per call"]
    for steps in (1, 4):
        dt = (steps - 0.5) * ts / 2              # steps - 1 full steps of ts / 2 and half a step
        plan = fl.flow_loss_plan(desc, R, t, dt, a.max_workspace_bytes)
        outs = dict(loss=torch.empty(2, device="cuda"), flow2d=torch.empty(R, 2, device="cuda"), g_weights=torch.empty_like(w))

        def raw_fwd():
            return fl.flow_loss_raw(desc, node.ws, node.flags, ro, rd, w, t, dt, cam, target, plan=plan, **outs)

        def raw_both():
            fl.flow_loss_backward_raw(desc, raw_fwd(), G)

        def autograd_form():
            return torch.autograd.grad(f.flow_loss(weights, dt, cam, target, weight_grad=False, max_workspace_bytes=a.max_workspace_bytes), params)

        def torch_ops():
            return torch.autograd.grad(torch_form(f, o, d, u, wl, t, dt, pose, focal, target), [wl] + params)

        for _ in range(3):
            raw_both(); autograd_form(); torch_ops()
        torch.cuda.synchronize()
        v_hip = float(raw_fwd()["loss"][0])
        v_ref = float(torch_form(f, o, d, u, wl, t, dt, pose, focal, target))
        assert abs(v_hip - v_ref) <= 1e-4 * abs(v_ref), (steps, v_hip, v_ref)
        tf, tb, ta, tt = (timed(fn, a.reps, a.rounds) for fn in (raw_fwd, raw_both, autograd_form, torch_ops))
        lines.append(f"{steps} RK2 step(s): raw forward {tf[0]:8.1f} [{tf[1]:.1f} .. {tf[2]:.1f}] | raw forward + backward {tb[0]:8.1f} [{tb[1]:.1f} .. {tb[2]:.1f}] | "
                     f"autograd form {ta[0]:8.1f} [{ta[1]:.1f} .. {ta[2]:.1f}] | torch form {tt[0]:8.1f} [{tt[1]:.1f} .. {tt[2]:.1f}] | torch / raw {tt[0] / tb[0]:.2f} | "
                     f"torch / autograd {tt[0] / ta[0]:.2f} | workspace {plan[1]} bytes, {plan[2]} chunk(s) of {plan[0]} | loss {v_hip:.6f} (torch {v_ref:.6f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
