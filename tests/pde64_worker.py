"""helper of tests/test_gpu_pde64.py (subprocess: the NVFI_* switches are read once per process): runs get_vel_loss on the device for the cases
named on the command line and saves, per case, the inputs, the kept mask, the first 64 Jacobians, the loss, the kept count, the 24 gradients, the
call's bookkeeping (out[0..3]: loss, kept count, sum div^2, sum transport^2; the eight counters), plus the 24 parameters of every model used.   python tests/pde64_worker.py OUT.npz CASE[,CASE...]

Cases: `head` (the bench field, 262 144 points, a moving velocity field), `B<P>` (field B, which keeps every point of its box: P points),
`bigz` (field B with the first layer of both nets scaled by 2.5 and the four hidden ones by 4: pre-activations up to 25-35, 32 768 points), `abi<P>` (field B, P points,
nvfi_pde_loss_ex through ctypes with the acceleration net's slots / one hidden layer of weight_net left NULL)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import bench  # noqa: E402
from helpers import make_model  # noqa: E402

dev = torch.device("cuda", 0)
_models = {}


def model(kind):
    if kind not in _models:
        if kind == "head":
            m = bench.build_scene(dev, 199, 128, True)
            with torch.no_grad():          # a velocity field that moves (the init is ~0: the gradients would be rounding noise), as tests/x6_bwd_check.py
                last = m.nvfi.vel_net.weight_net[-1][0]
                last.weight.mul_(6.0); last.bias.copy_(torch.tensor([0.5, -0.3, 0.2, 0.1, -0.2, 0.4], device=dev))
        else:
            m, _ = make_model("B")
            if kind == "bigz":
                with torch.no_grad():          # |z| grows from ~4 in the first layer to 25-35 in the last hidden one (x 2.5 everywhere reaches 5 only)
                    for net in (m.nvfi.vel_net.weight_net, m.nvfi.vel_net.a_weight_net):
                        net[1].weight.mul_(2.5)
                        for i in range(3, 7):
                            net[i][0].weight.mul_(4.0)
        m.nvfi.train()
        m.requires_grad_(True)
        _models[kind] = m
    return _models[kind]


def inputs(kind, P, seed):
    f = model(kind).nvfi
    ab = f.aabb.detach().cpu().numpy()
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(0, 1, (P, 3)) * (ab[1] - ab[0]) + ab[0]).astype(np.float32)
    tt = rng.uniform(0, 1, (P, 1)).astype(np.float32)
    return pts, tt


def run_case(name, out):
    if name.startswith("abi"):
        return run_abi(name, int(name[3:]), out)
    kind, P = ("head", 262144) if name == "head" else ("bigz", 32768) if name == "bigz" else ("B", int(name[1:]))
    m = model(kind)
    f = m.nvfi
    pts, tt = inputs(kind, P, P)
    if kind == "bigz":
        # with |z| of 25-35 the acceleration net has units within fp32 rounding of their ReLU kink at ~0.2 % of the points; float64 and the device
        # may take different sides there and the point's gradient jumps (1e-4 of the mean at 32 768 points): points within 4 x the worst-case fp32
        # rounding of a kink (6 % of them) are redrawn
        import pde64
        pts2, tt2 = inputs(kind, 2 * P, P + 1)
        ok = pde64.relu_margin(pde64.normalize_points(pts2, f.aabb.detach().cpu().numpy()), tt2[:, 0], pde64.as_params(f._pde_params(), dev)) > 4.0
        pts, tt = pts2[ok][:P], tt2[ok][:P]
        assert pts.shape[0] == P, int(ok.sum())
    m.zero_grad(set_to_none=True)
    f.pde_debug = 64
    try:
        lv = m.get_vel_loss(points=torch.from_numpy(pts).to(dev), t=torch.from_numpy(tt).to(dev))
        n = int(f.last_pde_n_kept)
        kept = f.last_pde_kept.cpu().numpy().astype(bool)
        jac = f.last_pde_jac.cpu().numpy()
    finally:
        f.pde_debug = 0
    assert n > 0, name
    lv.backward()
    torch.cuda.synchronize()
    out[f"{name}:model"] = np.array(kind)
    out[f"{name}:points"], out[f"{name}:t"], out[f"{name}:kept"], out[f"{name}:jac"] = pts, tt[:, 0], kept, jac
    out[f"{name}:loss"], out[f"{name}:n_kept"] = np.float64(lv.detach().cpu()), np.int64(n)
    out[f"{name}:split"] = np.array(bool(f.pde_split) and P <= 262144)      # a split call (nvfi_pde_loss_split with a side stream, one chunk)
    out[f"{name}:out"], out[f"{name}:counters"] = f.last_pde_out.cpu().numpy(), f.last_pde_counters.cpu().numpy()
    for i, p in enumerate(f._pde_params()):
        out[f"{name}:g{i}"] = p.grad.detach().cpu().numpy()
    save_model(kind, out)
    print(name, "kept", n, "of", P, "loss", float(out[f"{name}:loss"]), flush=True)


def run_abi(name, P, out):
    """the partial gradient sets of test_gpu_edges.py::test_pde_c_abi_with_partial_gradient_sets on field B"""
    from nvfi_amd import _lib
    L = _lib.lib()
    f = model("B").nvfi
    pts, tt = inputs("B", P, P)
    pts_d, tt_d = torch.from_numpy(pts).to(dev).contiguous(), torch.from_numpy(tt[:, 0].copy()).to(dev).contiguous()
    desc = f._desc()
    nb = C.c_int64(0)
    _lib.check(L.nvfi_pde_workspace_bytes(C.byref(desc), C.c_int64(P), C.byref(nb)))
    for drop in ("accel", "layer2"):
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        grads = [torch.zeros_like(p) for p in f._pde_params()]
        G = f._grads_struct_vel(grads)
        if drop == "accel":
            for i in range(6):
                G.aW[i] = None; G.ab[i] = None
        else:
            G.vW[2] = None; G.vb[2] = None
        o = torch.zeros(4, device=dev)
        cnt = torch.zeros(_lib.NCOUNTERS, dtype=torch.int64, device=dev)
        kept = torch.zeros(P, dtype=torch.uint8, device=dev)
        _lib.check(L.nvfi_pde_loss_ex(C.byref(desc), C.c_int64(P), _lib.ptr(pts_d), _lib.ptr(tt_d), C.c_float(1.0), _lib.ptr(o), C.byref(G),
                                      _lib.ptr(ws), C.c_int64(ws.numel()), _lib.ptr(cnt), _lib.ptr(kept), None, C.c_int64(0), None, None))
        torch.cuda.synchronize()
        key = f"{name}_{drop}"
        out[f"{key}:model"] = np.array("B")
        out[f"{key}:points"], out[f"{key}:t"], out[f"{key}:kept"] = pts, tt[:, 0], kept.cpu().numpy().astype(bool)
        out[f"{key}:loss"], out[f"{key}:n_kept"] = np.float64(o[0].cpu()), np.int64(round(float(o[1])))
        out[f"{key}:out"], out[f"{key}:counters"] = o.cpu().numpy(), cnt.cpu().numpy()
        for i, g in enumerate(grads):
            out[f"{key}:g{i}"] = g.cpu().numpy()
        print(key, "kept", int(out[f"{key}:n_kept"]), "of", P, flush=True)
    save_model("B", out)


def save_model(kind, out):
    if f"model:{kind}:aabb" in out:
        return
    f = model(kind).nvfi
    out[f"model:{kind}:aabb"] = f.aabb.detach().cpu().numpy()
    for i, p in enumerate(f._pde_params()):
        out[f"model:{kind}:p{i}"] = p.detach().cpu().numpy()


if __name__ == "__main__":
    res = {}
    for c in sys.argv[2].split(","):
        run_case(c, res)
    np.savez(sys.argv[1], **res)
