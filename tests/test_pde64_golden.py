"""The float64 restatement of the PDE term (tests/pde64.py) against the reference's goldens on the golden kept sets: this pins the yardstick that
tests/test_gpu_pde64.py holds the device kernels to.

Measured (CPU, float64): field A (1 143 kept points) loss rel err 7.5e-8, Jacobian rows 0-2 max abs err 4.8e-8 (max |J| 0.47, max rel err 1.1e-6
where |J| > 1e-2), gradients worst max(maxrel, rel_l2) 3.2e-7 (weight_net.7.0.weight); field B (4 096 kept points) loss rel err 0 (the golden is
fp32), Jacobian max abs err 7.3e-8 (max rel 9.8e-7), gradients worst 2.2e-7 (a_weight_net.5.0.weight).  The bounds below are about 3 x those,
three orders under the C oracle's (rtol 2e-4 on the loss, 5e-4 on the gradients, test_oracle_golden.py::test_pde_loss): what is left is the
goldens' own fp32 rounding."""
import os

import numpy as np
import pytest

import pde64
from conftest import GOLD, relerr

KINDS = ["A", "B"]


@pytest.fixture(scope="module")
def params():
    z = np.load(os.path.join(GOLD, "field_A.npz"))      # field B shares the velocity nets of field A
    return pde64.as_params([z["sd:nvfi." + n] for n in pde64.NAMES])


@pytest.mark.parametrize("kind", KINDS)
def test_pde64_matches_the_reference_goldens(gold, params, kind):
    aabb = np.load(os.path.join(GOLD, f"field_{kind}.npz"))["meta:aabb"]
    kept = gold[f"{kind}:pde:kept"]
    r = pde64.pde64(gold[f"{kind}:pde:points"], gold[f"{kind}:pde:t"], kept, params, aabb, n_jac=64)
    assert r["n_kept"] == int(kept.sum()) and r["n_kept"] > 1000
    np.testing.assert_allclose(r["loss"], float(gold[f"{kind}:pde:loss"][0]), rtol=3e-7)
    np.testing.assert_allclose(r["jac"], gold[f"{kind}:pde:jac64"][:, :3], rtol=3e-6, atol=2.5e-7)
    n = 0
    for k in gold.files:
        pre = f"{kind}:pde:grad:"
        if k.startswith(pre):
            e = relerr(r["grads"]["vel_net." + k[len(pre):]], gold[k])
            assert e < 1e-6, (k, e)
            n += 1
    assert n == (24 if kind == "A" else 8)


def test_pde64_sums_split_over_any_partition(params):
    """the drop-a-tile shift of the GPU file's self-checks (pde64.without) equals a full recomputation on the reduced kept set"""
    z = np.load(os.path.join(GOLD, "hotpath.npz"))
    aabb = np.load(os.path.join(GOLD, "field_B.npz"))["meta:aabb"]
    pts, t = z["B:pde:points"][:300], z["B:pde:t"][:300]
    kept = np.ones(300, bool)
    ref = pde64.pde64(pts, t, kept, params, aabb, chunk=128)
    drop = np.arange(64, 96)
    loss, g = pde64.without(ref, params, drop)
    k2 = kept.copy(); k2[drop] = False
    r2 = pde64.pde64(pts, t, k2, params, aabb)
    np.testing.assert_allclose(loss, r2["loss"], rtol=1e-12)
    for k in pde64.NAMES:
        np.testing.assert_allclose(g[k], r2["grads"][k], rtol=1e-9, atol=1e-12 * np.abs(r2["grads"][k]).max())
