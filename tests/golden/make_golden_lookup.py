#!/usr/bin/env python
"""Golden vectors of the differentiable field lookups (nvfi_density_grad, nvfi_appfeat_at, nvfi_appfeat_grad), generated from the REFERENCE
implementation (PyTorch CPU):
    python tests/golden/make_golden_lookup.py        (reference checkout as in make_golden.py)
The reference's compute_densityfeature / compute_appfeature (models/tensorf_keyframe.py:233-310) are plain torch code: called on points that
require grad, a loss on their outputs fills the .grad of the twelve planes, of basis_mat and of the points.  Fields: the two golden fields of
make_golden.py, A (K = 4) and B (K = 16), asserted equal to tests/golden/field_{A,B}.npz.  Writes tests/golden/lookup.npz (numbers only), per
field <kind>:
  xyzt (96, 4)                       the points: lookup64.point_mix - interior points, exact texel nodes (-1, +1, and 0 where G is odd), box faces,
                                     points out to 1.15 x the box, integer and fractional time rows, t' below -1 and above +1
  density:g (96), app:g (96, app_dim)   the random upstream gradients; the loss is sum(feat * g), one backward per family
  density:value (96), app:value (96, app_dim), <family>:g_xyzt (96, 4), <family>:grad:<tensor>   the reference's fp32 results
ASSERTS: every coordinate that is not a placed node keeps its fp32 texel coordinate at least 1e-4 from an integer, and on every placed node the
reference's expression of the texel coordinate (ATen: ((g + 1) / 2) * (W - 1)) and the device's ((g + 1) * ((W - 1) / 2)) are the SAME fp32
integer - so the two take every cell decision alike by construction and no case needs leaving out (an integer time row on which they differ
is redrawn as a fractional one); nothing reaches the velocity nets or the render MLP; both families see a non-zero t' gradient."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import lookup64 as l64  # noqa: E402
import render64 as r64  # noqa: E402

SEED = 4321
N = 96


def texel32(q, sizes):
    """(device's, ATen's) fp32 texel coordinates of the four columns"""
    q = np.asarray(q, np.float32)
    ours = np.stack([(q[:, c] + np.float32(1)) * np.float32((W - 1) / 2.0) for c, W in enumerate(sizes)], 1)
    aten = np.stack([((q[:, c] + np.float32(1)) / np.float32(2)) * np.float32(W - 1) for c, W in enumerate(sizes)], 1)
    return ours, aten


def points(rng, grid, K):
    q = l64.point_mix(rng, N, grid, K)
    sizes = list(grid) + [K]
    for _ in range(64):
        ours, aten = texel32(q, sizes)
        node = l64.texel_distance(q, grid, K) < 1e-4
        bad = node & ~((ours == aten) & (ours == np.rint(ours)))
        if not bad.any():
            break
        assert not bad[:, :3].any(), "a placed spatial node on which the two expressions differ"
        q[bad[:, 3], 3] = (rng.random(int(bad[:, 3].sum())) * 2 - 1).astype(np.float32)
    assert not bad.any()
    return q, node


def run_family(nv, q, g, family):
    f = nv.nvfi
    f.eval()
    nv.zero_grad(set_to_none=True)
    x = torch.from_numpy(q.copy()).requires_grad_(True)
    feat = f.compute_densityfeature(x)[:, 0] if family == "density" else f.compute_appfeature(x)
    (feat * torch.from_numpy(g)).sum().backward()
    named = dict(nv.named_parameters())
    names = l64.D_NAMES if family == "density" else l64.A_NAMES
    for k, p in named.items():
        assert (k[5:] in names) or p.grad is None, (family, k)          # nothing else is reached
    return dict(value=mg.npf(feat), g_xyzt=mg.npf(x.grad), grads={n: mg.npf(named["nvfi." + n].grad) for n in names})


def main():
    R = mg.import_reference()
    torch.set_num_threads(4)
    cfgA, nvA = mg.build_field(R, "A")
    shared = dict(vel_net=nvA.nvfi.vel_net.state_dict(), render=nvA.nvfi.renderModule.state_dict(), basis=nvA.nvfi.basis_mat.state_dict())
    cfgB, nvB = mg.build_field(R, "B", seed=77, shared_nets=shared)
    fx = {}
    for kind, nv in (("A", nvA), ("B", nvB)):
        f = nv.nvfi
        z = np.load(os.path.join(HERE, f"field_{kind}.npz"))
        sd = {k: mg.npf(v) for k, v in nv.state_dict().items()}
        for n in r64.PLANE_NAMES:
            assert np.array_equal(sd["nvfi." + n], z["sd:nvfi." + n]), (kind, n, "the rebuilt field is not the golden field")
        grid, K = [int(v) for v in f.gridSize], int(f.num_keyframes)
        rng = np.random.default_rng(SEED + (0 if kind == "A" else 1))
        q, node = points(rng, grid, K)
        dist = l64.texel_distance(q, grid, K)
        assert (dist[~node] >= 1e-4).all()
        assert (np.abs(q[:, :3]) > 1).any() and (q[:, 3] < -1).any() and (q[:, 3] > 1).any() and node[:, 3].sum() >= 4 and node[:, :3].sum() >= 6
        fx[f"{kind}:xyzt"] = q
        field = r64.Field({k: v for k, v in sd.items() if not k.startswith("nvfi.vel.vel_net.")}, {k[5:]: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("meta:")})
        for family, cols, fn in (("density", (), l64.density_lookup64), ("app", (int(f.app_dim),), l64.app_lookup64)):
            g = rng.standard_normal((N,) + cols).astype(np.float32)
            ref = run_family(nv, q, g, family)
            assert np.abs(ref["g_xyzt"][:, 3]).max() > 0
            fx[f"{kind}:{family}:g"] = g
            fx[f"{kind}:{family}:value"], fx[f"{kind}:{family}:g_xyzt"] = ref["value"], ref["g_xyzt"]
            for n, v in ref["grads"].items():
                fx[f"{kind}:{family}:grad:{n}"] = v
            y64, y32 = fn(field, q, g), fn(field, q, g, dtype=torch.float32)
            t64, t32, tr = l64.tensors(y64), l64.tensors(y32), l64.tensors(ref)
            for label in t64:
                e, b = l64.max_err(tr[label], t64[label]), l64.bound(t64[label], t32[label])
                print(f"{kind}:{family}:{label}: max |ref64| {np.abs(t64[label]).max():.3g}  reference - yardstick {e:.2e}  float32 floor "
                      f"{l64.max_err(t32[label], t64[label]):.2e}  bound {b:.2e}  {'ok' if e <= b else 'OUTSIDE'}")
    path = os.path.join(HERE, "lookup.npz")
    np.savez_compressed(path, **fx)
    print("wrote lookup.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
