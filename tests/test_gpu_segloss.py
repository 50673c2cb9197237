"""The segmentation objective on the GPU (nvfi_amd/utils/seg_loss.py over nvfi_knn_self / nvfi_segloss, csrc/segloss.hip) against the float64
yardstick tests/segloss64.py, which tests/test_segloss64_golden.py pins to the reference's outputs (tests/golden/segloss.npz).

Fixture cases: the loss block of train_segm.py:182-202 as written there - dynamic_loss(xyz, mask, flow), smooth_loss(xyz, mask, k, radius),
entropy_loss(mask) on (1, N, .) tensors - with only the import changed.
  neighbour tables: every row equals the golden's, except rows inside the near-tie band (every slot within 1e-5 relative of the golden's slot in
      float64 squared distance, a replaced slot counting as `radius`); those are counted and must stay <= 0.5 % of the points.  The golden stores
      the tables of two cases on every 4th row; the yardstick's brute-force search (pinned to the golden on those rows) is compared on ALL rows.
  losses, pc_transformed, d loss / d mask: against segloss64 in float64 ON THE DEVICE'S OWN TABLE; bound per quantity and case = 4 x the distance
      of segloss64 evaluated in float32 from itself in float64 (same case, same table), derived here, printed with the device's error.
  R, t: where the fixture's sigma_min / sigma_max of S_k is above the recorded floor; the NaN case gives the identity.
Run this file as the GPU suite does: under `timeout`, with -x, so that the run ends at the first fault."""
import os

import numpy as np
import pytest
import torch

import segloss64 as s64
from conftest import GOLD, maxrel, rel_l2
from test_segloss64_golden import BOUND as PIN, CASES, load_case

pytestmark = pytest.mark.gpu
MARGIN = 4.0
BAND_CAP = 5e-3


@pytest.fixture(scope="module")
def sgold():
    return np.load(os.path.join(GOLD, "segloss.npz"))


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()[None].requires_grad_(grad)


def _err(a, b):
    if np.ndim(b) == 0:
        return abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0 else abs(float(a))
    return max(maxrel(a, b), rel_l2(a, b))


def device_losses(pc, flow, mask, k, radius, norm):
    """the three reference calls, each with its own backward -> dict of numpy results + the device's neighbour table"""
    from nvfi_amd.utils import seg_loss as sl
    out = {}
    tp, tf = _t(pc), _t(flow)
    m = _t(mask, True)
    loss, pct = sl.dynamic_loss(tp, m, tf)
    loss.backward()
    out.update(dynamic=loss.item(), pc_transformed=pct[0].cpu().numpy(), g_dynamic=m.grad[0].cpu().numpy())
    m = _t(mask, True)
    loss = sl.smooth_loss(tp, m, k=k, radius=radius, loss_norm=norm)
    loss.backward()
    out.update(smooth=loss.item(), g_smooth=m.grad[0].cpu().numpy())
    m = _t(mask, True)
    loss = sl.entropy_loss(m)
    loss.backward()
    out.update(entropy=loss.item(), g_entropy=m.grad[0].cpu().numpy())
    idx, d2, rs, re = sl.knn_self(tp[0], k, radius, reverse=True, return_dist=True)
    out.update(idx=idx.cpu().numpy().astype(np.int64), d2=d2.cpu().numpy(), rev_start=rs.cpu().numpy(), rev_edge=re.cpu().numpy())
    K = mask.shape[1]
    R, t = sl.fit_motion_svd_batch(tp.repeat(K, 1, 1), (tp + tf).repeat(K, 1, 1), torch.from_numpy(np.ascontiguousarray(mask.T)).cuda())
    out.update(R=R.cpu().numpy(), t=t.cpu().numpy())
    return out


def check_tables(pc, k, radius, dev, label):
    """structure of the device's tables, and the table against the yardstick's search on every row -> rows inside the band"""
    N = pc.shape[0]
    idx = dev["idx"]
    assert idx.shape == (N, k) and idx.min() >= 0 and idx.max() < N
    yidx, _, _ = s64.knn_brute(pc, k, radius)
    differ, outside = s64.idx_mismatch(pc, radius, idx, yidx)
    print(f"[segloss] {label}: table differs from the brute-force search on {differ} of {N} rows ({outside} outside the band)")
    assert outside == 0 and differ <= max(BAND_CAP * N, 0), (label, differ, outside)
    # distances: ascending, finite exactly on the slots that are real neighbours, and those are the fp32 squared distances
    d2 = dev["d2"]
    real = np.isfinite(d2)
    assert (np.diff(np.where(real, d2, np.float32(3e38)), axis=1) >= 0).all() and (d2[real] <= np.float32(radius)).all()
    assert (idx[~real] == np.broadcast_to(idx[:, :1], idx.shape)[~real]).all()
    np.testing.assert_allclose(d2[real], s64.d2_64(pc, np.nonzero(real)[0], idx[real]), rtol=1e-5, atol=1e-12)
    # reverse lists: exactly the live edges, every list ascending
    rs, re = dev["rev_start"], dev["rev_edge"]
    live = np.nonzero((idx != np.arange(N)[:, None]).reshape(-1))[0]
    assert rs[0] == 0 and rs[-1] == live.size and (np.diff(rs) >= 0).all()
    tgt = idx.reshape(-1)[live]
    order = np.lexsort((live, tgt))
    assert np.array_equal(re[:live.size], live[order]) and np.array_equal(np.bincount(tgt, minlength=N), np.diff(rs))
    return differ


def check_against_yardstick(pc, flow, mask, k, radius, norm, dev, label, sv_ok=None):
    y = s64.segloss64(pc, flow, mask, dev["idx"], norm, 1e-5)
    y32 = s64.segloss64(pc, flow, mask, dev["idx"], norm, 1e-5, dtype=np.float32)
    bad, bounds = [], {}
    for q in ("dynamic", "smooth", "entropy", "pc_transformed", "g_dynamic", "g_smooth", "g_entropy"):
        bound, e = MARGIN * _err(y32[q], y[q]), _err(dev[q], y[q])
        bounds[q] = bound
        print(f"[segloss] {label}: {q}: device {e:.2e}, bound {bound:.2e} (= {MARGIN:g} x float32 evaluation)")
        if not e <= bound:
            bad.append((q, e, bound))
    ok = np.nan_to_num(y["sv"][:, 2] / y["sv"][:, 0], nan=0.0) > 1e-3 if sv_ok is None else sv_ok
    for q in ("R", "t"):
        if ok.any():
            bound, e = MARGIN * np.abs(y32[q][ok] - y[q][ok]).max(), np.abs(dev[q][ok] - y[q][ok]).max()
            print(f"[segloss] {label}: {q}: device {e:.2e}, bound {bound:.2e}")
            if not e <= bound:
                bad.append((q, e, bound))
    nan = np.isnan(y["sv"]).any(1)
    assert np.array_equal(dev["R"][nan], np.broadcast_to(np.eye(3, dtype=np.float32), dev["R"][nan].shape)) and not dev["t"][nan].any()
    assert not bad, (label, bad)
    return y, bounds


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(sgold, name):
    c = load_case(sgold, name)
    dev = device_losses(c["pc"], c["flow"], c["mask"], c["k"], c["radius"], c["loss_norm"])
    N = c["pc"].shape[0]
    differ, outside = s64.idx_mismatch(c["pc"], c["radius"], dev["idx"][c["idx_rows"]], c["idx"], float(sgold["band"]), points=c["idx_rows"])
    print(f"[segloss] {name}: table differs from the golden on {differ} of {len(c['idx_rows'])} stored rows ({outside} outside the band)")
    assert outside == 0 and differ <= BAND_CAP * N
    check_tables(c["pc"], c["k"], c["radius"], dev, name)
    assert float(sgold["sv_floor"]) == 1e-3
    y, bounds = check_against_yardstick(c["pc"], c["flow"], c["mask"], c["k"], c["radius"], c["loss_norm"], dev, name, sv_ok=c["sv_ok"])
    if name == "zerocol":
        assert np.isnan(y["sv"][2]).all() and np.array_equal(dev["R"][2], np.eye(3)) and not dev["t"][2].any()
    # and the golden's own numbers on the stored rows: the device's bound against the yardstick + the yardstick's pinned distance from the golden
    for i, q in enumerate(("dynamic", "smooth", "entropy")):
        assert _err(dev[q], c["losses"][i]) <= bounds[q] + PIN[q], (q, dev[q], c["losses"][i])
    for q in ("pc_transformed", "g_dynamic", "g_smooth", "g_entropy"):
        e = _err(dev[q][c["rows"]], c[q])
        print(f"[segloss] {name}: {q} against the golden (stored rows): {e:.2e}")
        assert e <= 2 * bounds[q] + PIN[q], (q, e)      # (2 x: the bound was taken over all rows, the error over a quarter of them)


def _cloud(N, K, seed, dup=False):
    rng = np.random.default_rng(seed)
    pc = ((rng.random((N, 3)) - 0.5) * (0.6 if N < 1000 else 1.6)).astype(np.float32)
    if dup and N >= 8:      # exact duplicates: a run of copies of one point and scattered pairs
        pc[N // 2:N // 2 + min(N // 4, 40)] = pc[0]
        n7 = len(pc[2::7])
        pc[1::7][:n7] = pc[2::7]
    z = rng.standard_normal((N, K)) * 2.0
    mask = np.exp(z - z.max(1, keepdims=True))
    mask = (mask / mask.sum(1, keepdims=True)).astype(np.float32)
    flow = (0.02 * rng.standard_normal((N, 3)) + np.array([0.03, 0.0, -0.01])).astype(np.float32)
    return pc, flow, mask


@pytest.mark.parametrize("N", [1, 2, 63, 65, 4097])
def test_ragged_sizes(N):
    pc, flow, mask = _cloud(N, 8, N)
    for k, radius, norm in ((4, 0.01, 1), (16, 0.1, 2)):
        dev = device_losses(pc, flow, mask, k, radius, norm)
        check_tables(pc, k, radius, dev, f"N={N},k={k}")
        if N >= 63:
            check_against_yardstick(pc, flow, mask, k, radius, norm, dev, f"N={N},k={k}")
        else:       # one or two points: every quantity is finite and the smoothness term sees at most the other point
            for q in ("dynamic", "smooth", "entropy", "g_dynamic", "g_smooth", "g_entropy", "pc_transformed"):
                assert np.isfinite(dev[q]).all(), (N, q)
            y = s64.segloss64(pc, flow, mask, dev["idx"], norm, 1e-5)
            for q in ("smooth", "entropy", "g_smooth", "g_entropy"):
                assert _err(dev[q], y[q]) <= 1e-5 or abs(float(np.max(np.abs(y[q])))) == 0, (N, q)


def test_duplicate_points():
    pc, flow, mask = _cloud(1500, 5, 77, dup=True)
    assert np.unique(pc, axis=0).shape[0] < 1500 - 40
    for k, radius, norm in ((4, 0.01, 1), (8, 0.02, 2)):
        dev = device_losses(pc, flow, mask, k, radius, norm)
        differ = check_tables(pc, k, radius, dev, f"duplicates,k={k}")
        assert differ == 0          # equal distances are ordered by index: nothing is left open
        check_against_yardstick(pc, flow, mask, k, radius, norm, dev, f"duplicates,k={k}")


def _fused(pc, flow, mask, k=4, radius=0.01, sw=0.1, ew=0.05):
    from nvfi_amd.utils import seg_loss as sl
    m = _t(mask, True)
    loss, parts = sl.segm_losses(_t(pc), m, _t(flow), k, radius, sw, ew)
    loss.backward()
    return loss.detach().clone(), parts.clone(), m.grad.clone()


def test_two_calls_are_bit_identical(sgold):
    c = load_case(sgold, "lattice_k4")
    a = _fused(c["pc"], c["flow"], c["mask"])
    for _ in range(3):
        b = _fused(c["pc"], c["flow"], c["mask"])
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    from nvfi_amd.utils import seg_loss as sl
    t1 = sl.knn_self(_t(c["pc"])[0], 16, 0.1, return_dist=True)
    t2 = sl.knn_self(_t(c["pc"])[0], 16, 0.1, return_dist=True)
    live = int(t1[2][-1])           # rev_edge holds rev_start[N] entries; the rest of the buffer is not written
    assert live == int(t2[2][-1]) and all(torch.equal(x, y) for x, y in zip(t1[:3], t2[:3])) and torch.equal(t1[3][:live], t2[3][:live])


def test_fused_equals_the_three_functions(sgold):
    """segm_losses = dynamic + smooth_w * smooth + entropy_w * entropy: the parts are the separate functions' values bit for bit (same kernels,
    same order), the total and the gradient agree to fp32 rounding of the weighted sum (a few ulp of the largest term)"""
    c = load_case(sgold, "lattice_k4")
    sw, ew = 0.1, 0.05
    loss, parts, g = _fused(c["pc"], c["flow"], c["mask"], c["k"], c["radius"], sw, ew)
    dev = device_losses(c["pc"], c["flow"], c["mask"], c["k"], c["radius"], 1)
    sep = np.array([dev["dynamic"], dev["smooth"], dev["entropy"]], np.float32)
    assert np.array_equal(parts[0].cpu().numpy(), sep)
    want = float(sep[0]) + sw * float(sep[1]) + ew * float(sep[2])
    assert abs(float(loss) - want) <= 4 * np.finfo(np.float32).eps * abs(want)
    # gradient: the fused row is ONE running sum of the dynamic term, K entropy terms and k + indegree smoothness terms; each addition rounds
    # by at most eps / 2 of the running magnitude, which the sum of the terms' magnitudes bounds
    indeg = np.diff(dev["rev_start"]).astype(np.float64)[:, None]
    N, k = dev["idx"].shape
    gw = dev["g_dynamic"].astype(np.float64) + sw * dev["g_smooth"] + ew * dev["g_entropy"]
    scale = np.abs(dev["g_dynamic"]) + ew * np.abs(dev["g_entropy"]) + sw * (k + indeg) / (N * k)
    assert (np.abs(g[0].cpu().numpy() - gw) <= (k + indeg + 4) * np.finfo(np.float32).eps * scale).all()


def test_graph_capture_replays_bit_identical(sgold):
    from nvfi_amd.utils import seg_loss as sl
    c = load_case(sgold, "lattice_k4")
    eager = _fused(c["pc"], c["flow"], c["mask"])
    tp, tf = _t(c["pc"]), _t(c["flow"])
    m = _t(c["mask"], True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):       # warm-up outside the capture (code objects, allocator)
        for _ in range(2):
            loss, parts = sl.segm_losses(tp, m, tf, 4, 0.01, 0.1, 0.05)
            m.grad = None
            loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, parts = sl.segm_losses(tp, m, tf, 4, 0.01, 0.1, 0.05)
        loss.backward()
    for _ in range(2):
        m.grad.zero_()          # (the captured backward accumulates into the captured .grad)
        parts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager[0]) and torch.equal(parts, eager[1]) and torch.equal(m.grad, eager[2])


def test_training_at_the_shipped_size():
    """BASELINE config 5 with the real objective: segm_points on the bench's bat-box field at 64^3 -> MaskField -> segm_losses -> backward ->
    Adam, 200 iterations on one draw of the points, the smoothness term switched on at `smooth_iter`.  The true loss falls, the mask stays a
    softmax, and the loss call returns while the stream still has earlier work queued (no host synchronisation inside it)."""
    import bench
    from nvfi_amd.models import MaskField
    from nvfi_amd.utils import segm_points
    from nvfi_amd.utils import seg_loss as sl
    model = bench.build_scene(torch.device("cuda"), 199, 128, True)
    f = model.nvfi
    f.eval()
    torch.manual_seed(3)
    xyz, flow, t = segm_points(f, n_sample_res=64, min_t=0.5, alpha_scale=10.0)
    n = int(xyz.shape[0])
    assert n > 2000
    torch.manual_seed(233)
    mf = MaskField(n_layer=4, n_dim=128, input_dim=3, skips=[], mask_dim=8).cuda()
    opt = torch.optim.Adam(mf.parameters(), lr=1e-3, betas=(0.9, 0.999))
    smooth_iter, sw = 100, 0.1
    pc, fl = xyz[None], flow[None]

    def true_loss(w):
        with torch.no_grad():
            return float(sl.segm_losses(pc, mf(xyz)[None], fl, 4, 0.01, w)[0])

    first = {0.0: true_loss(0.0), sw: true_loss(sw)}
    hist = []
    for it in range(1, 201):
        mask = mf(xyz)
        w = 0.0 if it < smooth_iter else sw
        if it == 150:       # queue ~0.1 s of work, then the loss + backward: they must return with the stream still busy
            torch.cuda.synchronize()
            torch.cuda._sleep(200_000_000)
        loss, parts = sl.segm_losses(pc, mask[None], fl, 4, 0.01, w)
        opt.zero_grad()
        loss.backward()
        if it == 150:
            assert not torch.cuda.current_stream().query(), "the loss step waited for the device"
        opt.step()
        hist.append(parts)
    hist = torch.cat(hist).cpu().numpy()
    last = {0.0: true_loss(0.0), sw: true_loss(sw)}
    print(f"[segloss] shipped size: {n} points, t = {t:.3f}; dynamic {first[0.0]:.5f} -> {last[0.0]:.5f}, with smoothness {first[sw]:.5f} -> {last[sw]:.5f}; "
          f"smooth {hist[0, 1]:.4f} -> {hist[-1, 1]:.4f}, entropy {hist[0, 2]:.4f} -> {hist[-1, 2]:.4f}")
    assert np.isfinite(hist).all()
    assert last[0.0] < first[0.0] and last[sw] < first[sw]
    with torch.no_grad():
        mask = mf(xyz)
    assert float(mask.min()) >= 0.0
    np.testing.assert_allclose(mask.sum(1).cpu().numpy(), 1.0, atol=1e-5)


def test_input_checks():
    from nvfi_amd.utils import seg_loss as sl
    pc, flow, mask = (_t(a) for a in _cloud(64, 8, 5))
    with pytest.raises(NotImplementedError):
        sl.dynamic_loss(pc.clone().requires_grad_(True), mask, flow)
    with pytest.raises(NotImplementedError):
        sl.dynamic_loss(pc, mask, flow.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        sl.smooth_loss(pc, mask, k=4, radius=0.01, loss_norm=3)
    # B > 1 loops over the batch: the mean of the per-cloud losses, gradients per cloud / B
    pc2, flow2, mask2 = (_t(a) for a in _cloud(64, 8, 6))
    mb = torch.cat([mask, mask2]).requires_grad_(True)
    lb = sl.smooth_loss(torch.cat([pc, pc2]), mb, k=4, radius=0.01) + sl.dynamic_loss(torch.cat([pc, pc2]), mb, torch.cat([flow, flow2]))[0] + sl.entropy_loss(mb)
    lb.backward()
    m1, m2 = mask.clone().requires_grad_(True), mask2.clone().requires_grad_(True)
    l1 = sl.smooth_loss(pc, m1, k=4, radius=0.01) + sl.dynamic_loss(pc, m1, flow)[0] + sl.entropy_loss(m1)
    l2 = sl.smooth_loss(pc2, m2, k=4, radius=0.01) + sl.dynamic_loss(pc2, m2, flow2)[0] + sl.entropy_loss(m2)
    (0.5 * (l1 + l2)).backward()
    assert abs(float(lb) - 0.5 * float(l1 + l2)) <= 1e-6 * abs(float(lb))
    torch.testing.assert_close(mb.grad, torch.cat([m1.grad, m2.grad]), rtol=1e-5, atol=1e-9)
