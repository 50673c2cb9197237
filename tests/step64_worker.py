"""helper of tests/test_gpu_step64.py (one process per launch mode: the NVFI_* switches and the stream set-up are read once per process): drives
bench.Step / bench.GraphedStep - the iteration that bench.py times - for one set-up step and three recorded iterations and saves, per iteration,
the state before it (every parameter of the optimiser, exp_avg, exp_avg_sq), what it consumed, what it produced and the state after it.
   python tests/step64_worker.py OUT.npz MODE

Scene: bench.build_scene(dev, 37, 64, True) - a 37-texel grid leaves a partial 4 x 4 and a partial 8 x 8 scatter tile on every axis -, the
velocity head made to move as in tests/pde64_worker.py; 1029 rays per render (one over four k_weights_bwd blocks' multiple and over a 256-thread
multiple), 16 417 = 32 x 513 + 1 collocation points.  Seeds as in tests/test_gpu_graph.py, set after the set-up step.
Modes:
  eager1       Step, cfg3, NVFI_OVERLAP=0: one stream
  eager3       Step, cfg3: PDE term, render 1 and render 2 on three streams
  shadow3      the same with live=False: the optimiser steps a shadow copy, the field stays put (what the headline times)
  record       GraphedStep.host_record() + body() eagerly: every scalar of the iteration is read from device memory
  replay       the same captured once and replayed three times (the capture recipe of test_graph_replay_follows_the_eager_iteration); the eager
               pass through the record that the recipe starts with belongs to the set-up here, so this mode's iterations are 2, 3, 4 of the schedule
  cfg2_eager   Step, radiance-only workload (use_vel False): the regulariser pass runs early on a side stream, recorded per call and asserted
  cfg2_replay  GraphedStep on that workload, replayed
The appearance masks and the PDE term's kept set are not returned by the fused calls.  After the three iterations the state before each one is
put back into the field and the same rays / points go through forward() / pde_loss(): the mask (kept set) is saved only if its count equals the
fused call's own counter.  The field is left with its final parameters."""
import copy
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import bench  # noqa: E402  (before anything initialises the GPU: its setdefault on the graph packet-capture switch has to take effect first)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODES = ("eager1", "eager3", "shadow3", "record", "replay", "cfg2_eager", "cfg2_replay")
GRID, SAMPLES, N_RAYS, N_PTS = 37, 64, 1029, 16417
VEL_BIAS = [0.5, -0.3, 0.2, 0.1, -0.2, 0.4]


def scene(device, cfg2=False):
    """the model of every mode (deterministic: the test rebuilds it on the CPU to read the configuration scalars)"""
    torch.manual_seed(7)
    m = bench.build_scene(device, GRID, SAMPLES, True)
    with torch.no_grad():
        last = m.nvfi.vel_net.weight_net[-1][0]
        last.weight.mul_(6.0); last.bias.copy_(torch.tensor(VEL_BIAS, device=last.bias.device))
    if cfg2:
        m.nvfi.use_vel = False
    return m


def _names(model):
    return {id(p): k[len("nvfi."):] for k, p in model.named_parameters(remove_duplicate=False) if not k.startswith("nvfi.vel.vel_net.")}


def _np(x):
    return x.detach().cpu().contiguous().numpy().copy()


def main(out_path, mode):
    assert mode in MODES, mode
    dev = torch.device("cuda", 0)
    cfg2 = mode.startswith("cfg2")
    graphed = mode in ("record", "replay", "cfg2_replay")
    replay = mode in ("replay", "cfg2_replay")
    live = mode != "shadow3"
    if mode == "eager1":                             # read by bench.Step when it is built
        os.environ["NVFI_OVERLAP"] = "0"
    else:
        os.environ.pop("NVFI_OVERLAP", None)
    torch.manual_seed(7); torch.cuda.manual_seed(7)
    model = scene(dev, cfg2)
    f = model.nvfi
    name_of = _names(model)
    order = [name_of[id(p)] for g in model.get_optparam_groups(0.02, 1e-3) for p in g["params"]]
    field_params = [p for g in model.get_optparam_groups(0.02, 1e-3) for p in g["params"]]
    step = bench.Step(model, dev, N_RAYS, N_PTS, 1, 0, "cfg2" if cfg2 else "cfg3", live=live)
    assert (step.streams is None) == (mode == "eager1" or cfg2), (mode, step.streams)
    opt_params = [p for g in step.opt.param_groups for p in g["params"]]
    assert len(opt_params) == len(order)
    stepped = [(n, p) for n, p in zip(order, opt_params) if p.grad is not None]
    reg_streams = []
    reg_call = f.regularizers_backward_

    def reg_spy(*a, **k):          # which stream the regulariser pass was issued on
        reg_streams.append(torch.cuda.current_stream().cuda_stream)
        return reg_call(*a, **k)
    f.regularizers_backward_ = reg_spy

    step()                                           # optimiser state, workspaces
    it0 = 1
    gs = None
    if graphed:
        gs = bench.GraphedStep(step)
        if replay:                                   # the recipe's eager pass through the record: first touch of the device-scalar path
            gs.host_record(); gs.body()
            it0 = 2
    torch.cuda.synchronize()
    torch.manual_seed(11); torch.cuda.manual_seed(11)
    step.gen.manual_seed(5); step.rng = np.random.default_rng(5)
    step.seed_override, step.draw_it = 5, 0          # nvfi_draw_batch: (seed, iteration) -> the pixel batches and collocation points
    out = {"mode": np.array(mode), "it0": np.int64(it0), "names": np.array([n for n, _ in stepped]), "cfg2": np.array(cfg2)}
    nb = 1 if cfg2 else 2
    R = N_RAYS

    def snap(tag, k):
        for n, p in stepped:
            st = step.opt.state[p]
            out[f"it{k}:{tag}:p:{n}"], out[f"it{k}:{tag}:m:{n}"], out[f"it{k}:{tag}:v:{n}"] = _np(p), _np(st["exp_avg"]), _np(st["exp_avg_sq"])
        if not live:
            for n, p in zip(order, field_params):
                out[f"it{k}:{tag}:field:{n}"] = _np(p)

    graph = None
    for k in range(3):
        torch.cuda.synchronize()
        snap("before", k)
        rng = copy.deepcopy(step.rng)
        n_reg = len(reg_streams)
        main_stream = torch.cuda.current_stream().cuda_stream
        if not graphed:
            loss = step()
        elif not replay:
            gs.host_record(); gs.body(); loss = gs.loss
        elif graph is None:
            gs.host_record()
            graph = torch.cuda.CUDAGraph(); graph.register_generator_state(step.gen)
            cap = torch.cuda.Stream(); cap.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=cap):
                gs.body()
            gs.graph = graph
            graph.replay(); loss = gs.loss
        else:
            loss = gs()
        torch.cuda.synchronize()
        # ---- what the iteration consumed
        if cfg2:
            t_host = [float(np.float32(float(rng.integers(0, 46)) / 60.0))]
        else:
            i = int(rng.integers(0, 46))
            while i % 3 == 0:
                i = int(rng.integers(0, 46))
            t_host = [float(np.float32(i / 60.0)), float(np.float32(3 * int(rng.integers(0, 16)) / 60.0))]
        out[f"it{k}:t"] = np.array(t_host, np.float64)
        if graphed:
            out[f"it{k}:t_rec"] = _np(gs.rec[0:2])[2 - nb:].astype(np.float64)
            jit = _np(gs.rec[gs.off_jit:gs.off_jit + nb * R])
            out[f"it{k}:rec_head"] = _np(gs.rec[:gs.HEAD + gs.n_hyper])
        else:
            jit = _np(step.jit_dev)
        for b in range(nb):
            out[f"it{k}:o{b}"], out[f"it{k}:d{b}"], out[f"it{k}:tg{b}"] = _np(step.d_ro[b]), _np(step.d_rd[b]), _np(step.d_tg[b])
            out[f"it{k}:u{b}"] = jit[b * R:(b + 1) * R].reshape(R, 1)
        if not cfg2:
            out[f"it{k}:pts"], out[f"it{k}:pt"] = _np(step.d_pts), _np(step.d_t)
        # ---- what it produced
        keys = [0, 1] if not cfg2 else [0]
        for b in keys:
            out[f"it{k}:rgb{b}"] = _np(step.last_rgb[b])
        cnts = gs.flags[-nb:] if graphed else step.counters[-nb:]
        for b in range(nb):
            out[f"it{k}:counters{b}"] = _np(cnts[b])
        out[f"it{k}:loss"] = np.float64(float(loss))
        out[f"it{k}:regs"] = _np(step.last_regs).astype(np.float64)
        if not cfg2:
            out[f"it{k}:lv"] = np.float64(float(step.last_lv))
            out[f"it{k}:pde_out"], out[f"it{k}:pde_counters"] = _np(f.last_pde_out).astype(np.float64), _np(f.last_pde_counters)
        snap("after", k)
        out[f"it{k}:flat_nonzero_bits"] = np.int64(int((step.bucket.flat.view(torch.int32) != 0).sum()))
        out[f"it{k}:sched"] = np.array([step.L1w, step.tvd, step.tva, step.vw], np.float64)
        out[f"it{k}:lr"] = np.array([g["lr"] for g in step.opt.param_groups for _ in g["params"]], np.float64)
        out[f"it{k}:adam_step"] = np.array([int(step.opt.state[p]["step"]) for _, p in stepped], np.int64)
        out[f"it{k}:reg_on_side_stream"] = np.array([s != main_stream for s in reg_streams[n_reg:]])
        print(mode, "iteration", it0 + k, "t", t_host, "loss", float(loss), "counters", [c[:4].tolist() for c in (out[f"it{k}:counters{b}"] for b in range(nb))],
              "" if cfg2 else f"pde kept {out[f'it{k}:pde_out'][1]:.0f} lv {float(step.last_lv):.6g}", flush=True)
    if gs is not None and replay:
        gs.check()
    # ---- the masks and the kept sets: the state before each iteration back into the field, the same inputs through forward() / pde_loss()
    f.regularizers_backward_ = reg_call
    thres = np.float32(f.rayMarch_weight_thres)
    final = [p.detach().clone() for p in field_params]
    with torch.no_grad():
        for k in range(3):
            if live:
                for n, p in zip(order, field_params):
                    if f"it{k}:before:p:{n}" in out:
                        p.copy_(torch.from_numpy(out[f"it{k}:before:p:{n}"]).to(dev))
            for b in range(nb):
                f.jitter_override = torch.from_numpy(out[f"it{k}:u{b}"]).to(dev)
                try:
                    w = f(float(out[f"it{k}:t"][b]), torch.from_numpy(out[f"it{k}:o{b}"]).to(dev), torch.from_numpy(out[f"it{k}:d{b}"]).to(dev), True)[3]
                finally:
                    f.jitter_override = None
                if int(f.last_counters[2]) == int(out[f"it{k}:counters{b}"][2]):
                    out[f"it{k}:mask{b}"] = _np(w) > thres
                else:
                    print(mode, k, b, "forward() masks", int(f.last_counters[2]), "samples, the fused call", int(out[f"it{k}:counters{b}"][2]), flush=True)
            if not cfg2:
                f.pde_debug = 1
                try:
                    f.pde_loss(torch.from_numpy(out[f"it{k}:pts"]).to(dev), torch.from_numpy(out[f"it{k}:pt"]).to(dev))
                    kept, n = _np(f.last_pde_kept).astype(bool), int(f.last_pde_n_kept)
                finally:
                    f.pde_debug = 0
                if n == int(round(out[f"it{k}:pde_out"][1])) and int(kept.sum()) == n:
                    out[f"it{k}:kept"] = kept
                else:
                    print(mode, k, "pde_loss() keeps", n, "points, the fused call", out[f"it{k}:pde_out"][1], flush=True)
        for p, q in zip(field_params, final):
            p.copy_(q)
    torch.cuda.synchronize()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
