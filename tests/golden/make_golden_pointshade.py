#!/usr/bin/env python
"""Golden vectors of differentiable point shading (nvfi_render_mlp_grad), generated from the REFERENCE implementation (PyTorch CPU):
    python tests/golden/make_golden_pointshade.py        (reference checkout as in make_golden.py)
The reference's MLPRender_PE.forward (models/tensorf_base.py:88-98) and SHRender (models/tensorf_model_utils.py:292-296) are plain torch code:
called on inputs that require grad, a loss on their colours fills the .grad of the inputs and of renderModule.mlp.  Fields: the golden fields of
make_golden.py, A and B (B shares A's render MLP; both asserted equal to tests/golden/field_{A,B}.npz), and D, the SH field of A's geometry - SHRender
has no parameters.  Writes tests/golden/pointshade.npz (numbers only), per field <kind>:
  xyz (48, 3), view (48, 3), feat (48, app_dim), g (48, 3)     pointshade64.inputs(field, 48, SEED[kind]); the loss is sum(rgb * g)
  rgb (48, 3), g_features, g_xyz, g_view, grad:<tensor>         the reference's fp32 results (g_xyz: zeros under SH, which does not read xyz)
ASSERTS: the ReLU condition of pointshade64.relu_margin on every case (a seed that misses it is replaced by hand here); nothing but the six MLP
tensors is reached."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import point64 as p64  # noqa: E402
import pointshade64 as s64  # noqa: E402
import render64 as r64  # noqa: E402

N = 48
SEED = {"A": 5101, "B": 5102, "D": 5103}


def run(module, xyz, view, feat, g, params):
    for p in params.values():
        p.grad = None
    x, v, fe = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (xyz, view, feat)]
    rgb = module(x, v, fe, {})
    (rgb * torch.from_numpy(g)).sum().backward()
    zero = lambda a, gr: np.zeros(a.shape, np.float32) if gr is None else mg.npf(gr)  # noqa: E731
    return dict(rgb=mg.npf(rgb), g_features=zero(fe, fe.grad), g_xyz=zero(x, x.grad), g_view=zero(v, v.grad),
                grads={k: mg.npf(p.grad) for k, p in params.items()})


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    fx = {}
    for kind, nv in (("A", nvA), ("B", nvB), ("D", nvA)):
        src = "A" if kind == "D" else kind
        z = np.load(os.path.join(HERE, f"field_{src}.npz"))
        sd = {k: mg.npf(v) for k, v in nv.state_dict().items()}
        for n in r64.MLP_NAMES:
            if "sd:nvfi." + n in z.files:
                assert np.array_equal(sd["nvfi." + n], z["sd:nvfi." + n]), (kind, n, "the rebuilt field is not the golden field")
        meta = {k[5:]: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("meta:")}
        field = p64.field_of({k: v for k, v in sd.items() if not k.startswith("nvfi.vel.vel_net.")}, meta, sh=kind == "D")
        xyz, view, feat, g = s64.inputs(field, N, SEED[kind])
        same, room = s64.relu_margin(field, xyz, view, feat)
        assert same and room >= 1.0, (kind, SEED[kind], same, room)
        named = dict(nv.named_parameters())
        params = {} if kind == "D" else {n: named["nvfi." + n] for n in r64.MLP_NAMES}
        nv.zero_grad(set_to_none=True)
        ref = run(R["SHRender"] if kind == "D" else nv.nvfi.renderModule, xyz, view, feat, g, params)
        for k, p in named.items():
            assert (k[5:] in params) or p.grad is None, (kind, k)          # nothing else is reached
        for k, a in (("xyz", xyz), ("view", view), ("feat", feat), ("g", g)):
            fx[f"{kind}:{k}"] = a
        tr = s64.tensors(ref)
        for label, v in tr.items():
            fx[f"{kind}:{label}"] = v
        t64 = s64.tensors(s64.shade64(field, xyz, view, feat, g))
        t32 = s64.tensors(s64.shade64(field, xyz, view, feat, g, dtype=torch.float32))
        for label in t64:
            e, b = s64.max_err(tr[label], t64[label]), s64.bound(t64[label], t32[label])
            print(f"{kind}:{label}: max |ref64| {np.abs(t64[label]).max():.3g}  reference - yardstick {e:.2e}  float32 floor "
                  f"{s64.max_err(t32[label], t64[label]):.2e}  bound {b:.2e}  relu room {room:.1f}  {'ok' if e <= b else 'OUTSIDE'}")
    path = os.path.join(HERE, "pointshade.npz")
    np.savez_compressed(path, **fx)
    print("wrote pointshade.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
