#!/usr/bin/env python
"""2-D mask supervision (field.mask_fit_backward_ / field.mask_loss / render_mse_backward_(target_mask=): nvfi_mask_loss_fwd + nvfi_mask_loss_bwd;
csrc/maskloss.hip) on the bench's bat scene (bench.build_scene: 199^3 grid, K = 16) with a K = 8 MaskField, 2 048 rays x 128 samples, timed on
the GPU:
  fit step               field.mask_fit_backward_: eval render + mask loss + chunked MaskField backward into kept .grad buffers - the hot loop of
                         fitting a MaskField to 2-D masks of a trained scene
  host-assembled fit     what exists without the term: an eval render with the MaskField attached, the host read of the masked count,
                         nvfi_render_export_masked, MaskField through its autograd boundary, torch index_add composite, torch cross-entropy and
                         autograd to the ten tensors
  fused term             nvfi_mask_loss_fwd + the chunked nvfi_mask_loss_bwd behind ONE live training render (the term's own cost, not the
                         render's): what render_mse_backward_(target_mask=) adds to a step
  host-assembled term    field._mask_map_train on the same live render + torch cross-entropy + autograd to the weights (a leaf) and the ten tensors
One process, warm-up, HIP events around `reps` calls, the median of `rounds` rounds; the masked count, workspace bytes and chunk count are printed.
    python tools/bench_maskloss.py [--out profiles/maskloss_timing.txt] [--max-workspace-bytes B]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS = 1e-5


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


def torch_ce(q, labels, K):
    """the contract's cross-entropy on a mask map in torch: one-hot labels in [0, K), mean over the rays"""
    return -(torch.log(q.gather(1, labels[:, None].long()) + EPS)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-workspace-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maskloss needs the GPU: there is no CPU fallback"
    import bench
    from nvfi_amd import _lib
    from nvfi_amd.models import MaskField
    from nvfi_amd.models.mask_field import _mask_desc
    from nvfi_amd.utils import mask_loss as ml
    model = bench.build_scene("cuda")
    f = model.nvfi
    K, R = 8, a.rays
    ts = float(f.tmax) / (int(f.num_keyframes) - 1)
    torch.manual_seed(0)
    mf = MaskField(mask_dim=K).cuda()
    params = mf._params()
    for p in params:
        p.grad = torch.zeros_like(p)
    bo, bd = bench.camera_bundle("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    sel = torch.randperm(bo.shape[0], device="cuda", generator=g)[:R]
    o, d = bo[sel].contiguous(), bd[sel].contiguous()
    u = torch.rand(R, device="cuda", generator=g)
    labels = torch.randint(0, K, (R,), device="cuda", generator=g, dtype=torch.int32)
    t = 1.25 * ts
    desc = f._desc()
    md = _mask_desc(mf, params)
    plan = ml.mask_loss_plan(desc, md, R, a.max_workspace_bytes)
    MG = ml.mask_grads_struct([p.grad for p in params])

    # ---- the fit step on a frozen scene
    model.eval()

    def fit():
        return f.mask_fit_backward_(t, o, d, labels, mask_field=mf, kind="ce", eps=EPS)

    def fit_host():
        f.mask_field = mf
        try:
            with torch.no_grad():
                w = f(t, o, d, True)[3]
            M = int(f.last_counters[2])                   # the host read the device path does without
            xyz = torch.empty(M, 3, device="cuda")
            idx = torch.empty(M, dtype=torch.int64, device="cuda")
            Rl, tl, flags = f._last_call
            _lib.check(_lib.lib().nvfi_render_export_masked(C.byref(desc), R, tl, flags, _lib.ptr(f._last_ws),
                                                            f._last_ws.numel(), M, _lib.ptr(xyz), _lib.ptr(idx), _lib.stream_ptr()))
        finally:
            f.mask_field = None
        q = torch.zeros(R, K, device="cuda").index_add(0, idx // w.shape[1], w.reshape(-1)[idx][:, None] * mf(xyz))
        loss = torch_ce(q, labels, K)
        return loss, torch.autograd.grad(loss, params)

    for _ in range(3):
        fit(); fit_host()
    torch.cuda.synchronize()
    v_fit, v_host = float(fit()[0]), float(fit_host()[0])
    assert abs(v_fit - v_host) <= 1e-4 * abs(v_host), (v_fit, v_host)
    M_eval = int(f.last_counters[2])
    t_fit, t_fit_host = timed(fit, a.reps, a.rounds), timed(fit_host, a.reps, a.rounds)

    # ---- the term behind one live training render
    model.train()
    f.mask_field = mf
    f.jitter_override = u.reshape(-1, 1).cpu()
    try:
        out = f(t, o, d, True)                            # (with the MaskField attached: _mask_map_train can export from this render)
    finally:
        f.jitter_override = None
    weights = out[3]
    node = weights.grad_fn
    w = node.saved_tensors[2]
    M_train = int(f.last_counters[2])
    outs = dict(loss=torch.empty(2, device="cuda"), mask_map=torch.empty(R, K, device="cuda"), g_weights=torch.empty_like(w))
    ws = torch.empty(plan[1], dtype=torch.uint8, device="cuda")

    def term_fwd():
        return ml.mask_loss_raw(desc, md, node.ws, node.flags, w, t, labels, kind="ce", eps=EPS, plan=plan, workspace=ws, **outs)

    def term():
        ml.mask_loss_backward_raw(md, term_fwd(), MG)

    wl = w.detach().clone().requires_grad_(True)

    def term_host():
        q = f._mask_map_train(R, wl)
        return torch.autograd.grad(torch_ce(q, labels, K), [wl] + params)

    for _ in range(3):
        term(); term_host()
    torch.cuda.synchronize()
    v_term = float(term_fwd()["loss"][0])
    v_term_host = float(torch_ce(f._mask_map_train(R, wl), labels, K))
    assert abs(v_term - v_term_host) <= 1e-4 * abs(v_term_host), (v_term, v_term_host)
    t_fwd, t_term, t_term_host = timed(term_fwd, a.reps, a.rounds), timed(term, a.reps, a.rounds), timed(term_host, a.reps, a.rounds)
    f.mask_field = None
    fmt = lambda x: f"{x[0]:8.1f} [{x[1]:.1f} .. {x[2]:.1f}]"
    lines = [f"mask loss, K = {K}, R = {R} rays x {w.shape[1]} samples, bat scene {f.gridSize.tolist()} K = {int(f.num_keyframes)}; {torch.cuda.get_device_name(0)}; "
             f"max_workspace_bytes = {a.max_workspace_bytes}; HIP events, median of {a.rounds} rounds x {a.reps} calls [min .. max], us per call",
             f"fit step (eval render, {M_eval} masked samples): mask_fit_backward_ {fmt(t_fit)} | host-assembled {fmt(t_fit_host)} | host / fused {t_fit_host[0] / t_fit[0]:.2f} | "
             f"loss {v_fit:.6f} (host {v_host:.6f})",
             f"term behind a live training render ({M_train} masked samples): raw forward {fmt(t_fwd)} | raw forward + backward {fmt(t_term)} | "
             f"host-assembled {fmt(t_term_host)} | host / fused {t_term_host[0] / t_term[0]:.2f} | loss {v_term:.6f} (host {v_term_host:.6f})",
             f"workspace {plan[1]} bytes, {plan[2]} chunk(s) of {plan[0]} entries of the {R * w.shape[1]} capacity"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
