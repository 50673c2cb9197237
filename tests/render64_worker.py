"""helper of tests/test_gpu_render64.py (subprocess: the NVFI_* switches are read once per process): runs one training render + backward on the
device for the cases named on the command line and saves, per case, the inputs (rays, jitter, time, loss data), the maps, last_counters, the loss
and the 31 gradient tensors.   python tests/render64_worker.py OUT.npz CASE[,CASE...]

Scenes (scene(): also imported by the test, which rebuilds the same parameters on the CPU for the float64 reference): `head`, the bench field
(199^3, K = 16, 128 samples per ray) with a velocity head that moves; `B` / `A`, the golden fields.
Cases:
  head_nonkey / head_key   2048 rays of the bench camera bundle through render_mse_backward_ (white background, explicit jitter) at t = 19/60
                           (one RK2 step) / t = 0.3 (a keyframe): the calls bench.py times
  head_autograd            the head_nonkey rays through forward() + loss.backward() with the golden-style loss (depth, acc and weight terms)
  head_extrap              the same through render_mse_backward_ at t = 0.83, past the last keyframe: four RK2 steps
  m<N> / k<N>              field B (m0: the bench field), rays SELECTED from a pool (768 grazing rays and the 256 golden rays under six jitter draws; a sub-batch renders bit-identically) so
                           that the appearance-masked count (last_counters[2]) / the RK2 list (last_counters[1]) is exactly N; autograd path
  r<N>                     field B, the first N golden rays of the pool (N = 1, 3, 4, 5: k_weights_bwd takes four rays per block), or N = 2049,
                           8192, 8193 golden rays repeated under fresh jitter (PROLOGUE_MAX_RAYS = 8192), autograd path
  big686                   the largest shipped configuration (199^3, 686 samples per ray): the 2048-ray chunk runs, a fixed 256-ray subset is the case
  big_preact               field B with the render MLP's first layer x 2.5 and hidden layer x 4, 256 rays that keep 4 x the rounding bound from a kink
SH shading (scene `D`: helpers.sh_model, field A's geometry with shadingMode "SH"; `Dclamp`: the same with basis_mat.weight x 12; K = 4, tmax = 0.75):
  shD_nonkey / shD_key / shD_extrap     the 256 golden rays of field A through forward() + backward() with the golden-style loss at t = 19/60 (one
                           RK2 step), t = 0.25 (a keyframe) and t = 0.95 (past tmax, two RK2 steps)
  shD_fused_nonkey / shD_fused_key      the same rays through render_mse_backward_ (the six render-MLP slots of the gradient struct are empty)
  shm<N> / shr<N>          as m<N> / r<N>, on scene D with the pool of field A's rays
  shclamp / shclamp_fused  scene Dclamp, 256 rays of a 512-ray pool (the golden rays of field A under fresh jitter): a quarter of the composited
                           channels sit at the upper clamp, a fifth of the sample colours are dead; rays with a sample or channel within 4 x its
                           rounding bound of a kink (render64.relu_margin's SH form) are replaced by the next of the pool, and counted
In the small selections (N <= 129) only rays are used whose weights all keep 1.2e-5 from the appearance threshold on the device."""
import os
import sys

import numpy as np
import torch

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))

T_NONKEY, T_KEY, T_EXTRAP = 19.0 / 60.0, 0.3, 0.83
T_KEY_A, T_EXTRAP_A = 0.25, 0.95          # field A's geometry (K = 4, tmax = 0.75): a keyframe, and a time past tmax two RK2 steps from it
CLAMP_SCALE, CLAMP_POOL = 12.0, 512
RAYS_OF = {"D": "A", "Dclamp": "A"}       # the golden rays a scene is looked at through
_models = {}
_pool = {}


def scene(kind, device):
    """the model of a case family on `device` (deterministic: the test process rebuilds it on the CPU)"""
    import bench
    from helpers import make_model
    if kind == "head":
        m = bench.build_scene(device, 199, 128, True)
        with torch.no_grad():          # a velocity field that moves (the init is ~0), as tests/pde64_worker.py
            last = m.nvfi.vel_net.weight_net[-1][0]
            last.weight.mul_(6.0); last.bias.copy_(torch.tensor([0.5, -0.3, 0.2, 0.1, -0.2, 0.4], device=last.bias.device))
    elif kind == "big":            # the largest shipped configuration (tests/test_gpu_edges.py::test_largest_shipped_configuration) with a moving velocity field
        from nvfi_amd.models import NVFi
        torch.manual_seed(233)
        m = NVFi(bench.bat_cfg(1024, True), "cpu", torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]]), [199, 199, 199], [1.0, 8.0])
        with torch.no_grad():
            for i in range(3):
                p = m.nvfi.density_plane_space[i]
                H, W = p.shape[-2:]
                yy = torch.linspace(-1, 1, H)[:, None]; xx = torch.linspace(-1, 1, W)[None, :]
                p.mul_((3.2 * torch.sqrt(torch.exp(-xx ** 2 / (2 * 0.35 ** 2)) * torch.exp(-yy ** 2 / (2 * 0.35 ** 2))))[None, None])
            last = m.nvfi.vel_net.weight_net[-1][0]
            last.weight.mul_(6.0); last.bias.copy_(torch.tensor([0.5, -0.3, 0.2, 0.1, -0.2, 0.4]))
        m = m.to(device)
        assert m.nvfi.nSamples == 686, m.nvfi.nSamples
    elif kind in ("D", "Dclamp"):
        from helpers import sh_model
        m = sh_model(device)
        if kind == "Dclamp":           # SH colours far over 1 and far under 0: the clamp of the composite and the dead ReLU are taken
            with torch.no_grad():
                m.nvfi.basis_mat.weight.mul_(CLAMP_SCALE)
    else:
        m, _ = make_model("B" if kind == "bigz" else kind, device)
        if kind == "bigz":             # large pre-activations of the render MLP: first layer x 2.5, hidden layer x 4
            with torch.no_grad():
                m.nvfi.renderModule.mlp[0].weight.mul_(2.5)
                m.nvfi.renderModule.mlp[2].weight.mul_(4.0)
    m.nvfi.train()
    m.requires_grad_(True)
    return m


def head_rays(n=2048, seed=4):
    import bench
    o, d = bench.camera_bundle(torch.device("cpu"))
    idx = np.random.default_rng(seed).integers(0, o.shape[0], n)
    return o[idx].contiguous().numpy(), d[idx].contiguous().numpy()


def pool_rays(kind="B", reps=6):
    """the golden rays of the field under `reps` jitter draws (head: the headline rays and their jitter)"""
    if kind == "head":
        o, d = head_rays()
        return o, d, np.random.default_rng(5).uniform(0, 1, (o.shape[0], 1)).astype(np.float32)
    from conftest import GOLD
    kind = RAYS_OF.get(kind, kind)
    z = np.load(os.path.join(GOLD, "hotpath.npz"))
    o, d = np.tile(z[f"{kind}:rays_o"], (reps, 1)), np.tile(z[f"{kind}:rays_d"], (reps, 1))
    rng = np.random.default_rng(11)
    u = rng.uniform(0, 1, (o.shape[0], 1)).astype(np.float32)
    # grazing rays from the same camera position towards points near the edges of the box: short chords, lists of a few samples per ray
    ab = np.load(os.path.join(GOLD, f"field_{kind}.npz"))["meta:aabb"].reshape(2, 3).astype(np.float64)
    q = rng.uniform(-1, 1, (768, 3))
    ax = rng.integers(0, 3, 768)
    q[np.arange(768), ax] = np.sign(q[np.arange(768), ax]) * rng.uniform(0.97, 1.0, 768)
    q[np.arange(768), (ax + 1) % 3] = np.sign(q[np.arange(768), (ax + 1) % 3]) * rng.uniform(0.9, 1.03, 768)
    tgt = (q + 1) / 2 * (ab[1] - ab[0]) + ab[0]
    og = np.tile(o[:1], (768, 1))
    dg = tgt - og
    dg = (dg / np.linalg.norm(dg, axis=1, keepdims=True)).astype(np.float32)
    return (np.concatenate([og, o]), np.concatenate([dg, d]), np.concatenate([rng.uniform(0, 1, (768, 1)).astype(np.float32), u]))


def big_rays(N, kind="B"):
    """N rays for the ray-count cases: the golden rays of field B (or `kind`), repeated under fresh jitter"""
    from conftest import GOLD
    z = np.load(os.path.join(GOLD, "hotpath.npz"))
    reps = (N + 255) // 256
    o, d = np.tile(z[f"{kind}:rays_o"], (reps, 1))[:N], np.tile(z[f"{kind}:rays_d"], (reps, 1))[:N]
    return o, d, np.random.default_rng(13).uniform(0, 1, (N, 1)).astype(np.float32)


def loss_data(R, S, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (R, 3)).astype(np.float32), (rng.uniform(0, 1, (R, S)) * 0.01).astype(np.float32)


def model(kind):
    if kind not in _models:
        _models[kind] = scene(kind, torch.device("cuda", 0))
    return _models[kind]


def _run(name, kind, o, d, u, t, fused, out):
    from helpers import named_grads
    dev = torch.device("cuda", 0)
    m = model(kind)
    f = m.nvfi
    R, S = o.shape[0], f.nSamples
    target, gw = loss_data(R, S, R)
    m.zero_grad(set_to_none=True)
    od, dd, ud, tg = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (o, d, u, target))
    if fused:
        for p in f._render_params():
            if p is not None:          # (an SH field: the six render-MLP slots are empty)
                p.grad = torch.zeros_like(p)
        loss, rgb = f.render_mse_backward_(t, od, dd, tg, white_bg=True, jitter=ud.reshape(-1))
        torch.cuda.synchronize()
        maps = dict(rgb=rgb)
        cnt_fused = f.last_counters.cpu().numpy()
        # the fused driver keeps its weight map to itself: the same rays through a forward() of their own show the appearance mask (accepted as
        # the fused call's only if the masked counts agree)
        f.jitter_override = ud
        try:
            with torch.no_grad():
                w = f(t, od, dd, True)[3]
        finally:
            f.jitter_override = None
        if int(f.last_counters[2]) == int(cnt_fused[2]):
            maps["weights"] = w
        else:
            print(name, "the forward() of the same rays masks", int(f.last_counters[2]), "samples, the fused call", int(cnt_fused[2]),
                  ": its mask is not observable, the test falls back to the yardstick's own", flush=True)
        f.last_counters = torch.from_numpy(cnt_fused)
    else:
        f.jitter_override = ud
        try:
            rgb, depth, acc, w, _ = f(t, od, dd, True)
        finally:
            f.jitter_override = None
        loss = torch.nn.functional.mse_loss(rgb, tg) + 0.01 * depth.mean() + 0.02 * (acc ** 2).mean() + (w * torch.from_numpy(gw).to(dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
        maps = dict(rgb=rgb, depth=depth, acc=acc, weights=w)
    cnt = f.last_counters.cpu().numpy()
    out[f"{name}:model"], out[f"{name}:fused"], out[f"{name}:t"] = np.array(kind), np.array(fused), np.float64(t)
    out[f"{name}:rays_o"], out[f"{name}:rays_d"], out[f"{name}:u"], out[f"{name}:target"] = o, d, u, target
    if not fused:
        out[f"{name}:gw"] = gw
    for k, v in maps.items():
        out[f"{name}:{k}"] = v.detach().cpu().numpy()
    out[f"{name}:counters"], out[f"{name}:loss"] = cnt, np.float64(loss.detach().cpu())
    out[f"{name}:fork"] = np.array(bool(f.fork_backward))
    for k, g in named_grads(m).items():
        if g is not None:
            out[f"{name}:g:{k}"] = g
    if f"check:{kind}" not in out:
        out[f"check:{kind}"] = np.array([float(p.detach().double().abs().sum()) for _, p in sorted(named_grads_params(m))])
    print(name, "R", R, "counters", cnt[:4].tolist(), "loss", float(out[f"{name}:loss"]), flush=True)


def named_grads_params(m):
    return [(k, p) for k, p in m.named_parameters() if not k.startswith("nvfi.vel.vel_net.")]


def pool(kind="B"):
    """per pool ray, on the device: the masked count, the valid and in-gate counts (fp32 coordinates, as the yardstick decides them) and whether
    every weight keeps 1.2e-5 from the appearance threshold"""
    if kind not in _pool:
        import render64
        from helpers import field_state
        m = model(kind)
        f = m.nvfi
        o, d, u = pool_rays(kind)
        dev = torch.device("cuda", 0)
        f.jitter_override = torch.from_numpy(u).to(dev)
        try:
            with torch.no_grad():
                w = f(T_NONKEY, torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), True)[3].cpu().numpy()
        finally:
            f.jitter_override = None
        fld = render64.Field(*field_state(m))
        smp = render64.sample_rays(fld, o, d, u)
        gate = smp["valid"] & ~((smp["xn"] < fld.lo) | (smp["xn"] > fld.hi)).any(-1)
        thr = np.float32(fld.thres)
        _pool[kind] = dict(o=o, d=d, u=u, masked=(w > thr).sum(1), valid=smp["valid"].sum(1).numpy(), gate=gate.sum(1).numpy(),
                           margin=np.abs(w.astype(np.float64) - float(thr)).min(1), clear=(np.abs(w.astype(np.float64) - float(thr)) > 1.2e-5).all(1))
    return _pool[kind]


def clamp_rays(fld):
    """the 256 rays of shclamp and how many pool rays were passed over: decided by the yardstick alone (CPU or device, float64)"""
    import render64
    o, d, u = big_rays(CLAMP_POOL, "A")
    ms, mr = render64.relu_margin(fld, o, d, T_NONKEY, u, device="cuda" if torch.cuda.is_available() else "cpu")
    good = (ms > 4.0).all((1, 2)) & (mr > 4.0).all(1)
    ok = np.nonzero(good)[0][:256]
    assert len(ok) == 256, len(ok)
    return o[ok], d[ok], u[ok], int(ok[-1] + 1 - 256), int(ok[-1] + 1)


def run_sh_case(name, out):
    from helpers import field_state, select_rays
    import render64
    if name.startswith("shD_"):
        o, d = (np.load(os.path.join(root, "tests", "golden", "hotpath.npz"))[f"A:rays_{k}"] for k in "od")
        u = np.random.default_rng(17).uniform(0, 1, (o.shape[0], 1)).astype(np.float32)
        t = {"nonkey": T_NONKEY, "key": T_KEY_A, "extrap": T_EXTRAP_A}[name.split("_")[-1]]
        return _run(name, "D", o, d, u, t, "_fused_" in name, out)
    if name.startswith("shclamp"):
        o, d, u, redrawn, seen = clamp_rays(render64.Field(*field_state(model("Dclamp"))))
        out[f"{name}:redrawn"], out[f"{name}:pool_seen"] = np.int64(redrawn), np.int64(seen)
        return _run(name, "Dclamp", o, d, u, T_NONKEY, name.endswith("_fused"), out)
    N = int(name[3:])
    p = pool("D")
    if name[2] == "r":
        sel = 768 + np.arange(N)
    else:
        sel = select_rays(p["masked"], N, (p["valid"] > 0) & (p["clear"] if N <= 129 else True))
        assert sel is not None, (name, "no selection of pool rays reaches the count")
    _run(name, "D", p["o"][sel], p["d"][sel], p["u"][sel], T_NONKEY, False, out)


def run_case(name, out):
    from helpers import select_rays
    if name.startswith("sh"):
        return run_sh_case(name, out)
    if name.startswith("head_"):
        o, d = head_rays()
        u = np.random.default_rng(5).uniform(0, 1, (o.shape[0], 1)).astype(np.float32)
        t = {"head_nonkey": T_NONKEY, "head_autograd": T_NONKEY, "head_key": T_KEY, "head_extrap": T_EXTRAP}[name]
        return _run(name, "head", o, d, u, t, name != "head_autograd", out)
    if name == "big686":
        # the full 2048-ray chunk of the 686-sample configuration runs (finite, counters), then a fixed 256-ray subset as a call of its own
        import bench
        o, d = bench.camera_bundle(torch.device("cpu"))
        idx = np.random.default_rng(4).integers(0, o.shape[0], 2048)
        o, d = o[idx].contiguous().numpy(), d[idx].contiguous().numpy()
        u = np.random.default_rng(6).uniform(0, 1, (2048, 1)).astype(np.float32)
        full = {}
        _run("full", "big", o, d, u, T_NONKEY, False, full)
        assert all(np.isfinite(v).all() for k, v in full.items() if k.startswith("full:g:")) and int(full["full:counters"][0]) > 0.3 * 2048 * 686
        out["big686:full_counters"] = full["full:counters"]
        sub = np.sort(np.random.default_rng(7).choice(2048, 256, replace=False))
        return _run(name, "big", o[sub], d[sub], u[sub], T_NONKEY, False, out)
    if name == "big_preact":
        # rays of field B under the scaled render MLP; rays with a masked sample within 4 x the fp32 rounding bound of a ReLU kink
        # (render64.relu_margin, by the yardstick) are replaced by the next ones of the pool
        import render64
        from helpers import field_state
        o, d, u = big_rays(2048)
        mg = render64.relu_margin(render64.Field(*field_state(model("bigz"))), o, d, T_NONKEY, u, device="cuda")
        ok = np.nonzero((mg > 4.0).all(1))[0][:256]
        assert len(ok) == 256, len(ok)
        out["big_preact:redrawn"] = np.int64(ok[-1] + 1 - 256)
        return _run(name, "bigz", o[ok], d[ok], u[ok], T_NONKEY, False, out)
    N = int(name[1:])
    if name[0] == "r" and N > 5:
        o, d, u = big_rays(N)
        return _run(name, "B", o, d, u, T_NONKEY, False, out)
    kind = "head" if name == "m0" else "B"       # field B's density floor (softplus(-5) over a step) masks every valid sample: no ray of it has none
    p = pool(kind)
    if name[0] == "r":
        sel = 768 + np.arange(N)          # the first golden rays (the pool starts with 768 grazing rays)
    else:
        counts = p["masked"] if name[0] == "m" else p["gate"]
        usable = (p["valid"] > 0) & (p["clear"] if N <= 129 else True)
        if N == 0:
            # the bench field's density floor gives weights of 9.6e-5 - 9.9e-5, so no ray of it keeps 1.2e-5 from the threshold: the ray with
            # nothing masked that stays farthest from it is taken (3e-6 or so; the test still asserts that no sample changes side)
            zero = np.nonzero((p["valid"] > 0) & (counts == 0))[0]
            assert len(zero), "no ray with valid samples and nothing masked"
            sel = zero[np.argsort(-p["margin"][zero])[:1]]
        else:
            sel = select_rays(counts, N, usable)
            assert sel is not None, (name, "no selection of pool rays reaches the count")
    _run(name, kind, p["o"][sel], p["d"][sel], p["u"][sel], T_NONKEY, False, out)


if __name__ == "__main__":
    res = {}
    for c in sys.argv[2].split(","):
        run_case(c, res)
    np.savez(sys.argv[1], **res)
