"""bench.py --dump-outputs: what the timed step returned, as float32 .npy files under a size budget, sampled the same way in every run."""
import os

import numpy as np
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


class _FakeStep:
    def __init__(self):
        g = torch.Generator().manual_seed(0)
        self.params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 5_000_000, 4_000_000, 7)]
        self.opt = torch.optim.Adam([dict(params=self.params[:2], lr=0.02), dict(params=self.params[2:], lr=1e-3)])
        for p in self.params:
            p.grad = torch.ones_like(p)
        self.opt.step()
        self.last_rgb = {1: torch.rand(16, 3, generator=g), 0: torch.rand(16, 3, generator=g)}
        self.last_lv = torch.tensor(0.25)
        self.last_regs = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)


def test_step_outputs_are_float32_sampled_and_repeatable(tmp_path):
    import bench
    step = _FakeStep()
    a = bench.step_outputs(step, torch.tensor(0.5))
    b = bench.step_outputs(step, torch.tensor(0.5))
    assert set(a) == {"loss", "rgb_render0", "rgb_render1", "loss_vel", "regularizers"} | {f"param_{i:02d}" for i in range(4)} \
        | {f"adam_exp_avg_{i:02d}" for i in range(4)}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["param_00"], step.params[0].detach().numpy())          # small tensors whole
    np.testing.assert_array_equal(a["rgb_render1"], step.last_rgb[1].numpy())
    big = a["param_01"]
    assert 0 < big.size < step.params[1].numel()                                            # large ones sampled ...
    assert np.isin(big, step.params[1].detach().numpy()).all()                              # ... from their own elements
    assert sum(v.size for k, v in a.items() if k.startswith(("param_", "adam_"))) * 4 <= bench.DUMP_SAMPLED_BYTES
    bench.write_outputs(str(tmp_path / "d"), a)
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted(k + ".npy" for k in a)
    total = 0
    for f in files:
        x = np.load(tmp_path / "d" / f)
        assert x.dtype == np.float32
        total += x.nbytes
    assert total <= 64 << 20
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "regularizers.npy"), [1.0, 2.0, 3.0])


def test_parameter_and_moment_samples_hold_the_same_elements():
    import bench
    p = torch.nn.Parameter(torch.zeros(6_000_000))
    opt = torch.optim.Adam([p], lr=0.02)
    p.grad = torch.arange(p.numel(), dtype=torch.float32)        # exp_avg = 0.1 x the element index after one step
    opt.step()
    step = type("S", (), {"opt": opt})()
    out = bench.step_outputs(step, None)
    idx = np.rint(out["adam_exp_avg_00"].astype(np.float64) / 0.1)
    assert 0 < idx.size < p.numel() and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(out["param_00"], p.detach().numpy()[idx.astype(np.int64)])
