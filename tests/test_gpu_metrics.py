"""The evaluation metrics on the GPU (nvfi_amd/utils/metrics.py, metric_segm.py over nvfi_ssim / nvfi_segm_confusion, csrc/metrics.hip) against the
float64 yardstick tests/metrics64.py, which tests/test_metrics_golden.py pins to the reference's outputs (tests/golden/metrics.npz).

  confusion: counts and predicted labels exact; conf_sum within 1e-12 relative (fp64 sums of the same fp32 values in another order); every
      number of the full evaluator against the golden within the CPU file's bounds (check_summary there).
  SSIM mean and cs against the yardstick: bound = 4 x the reference's own fp32 distance from the yardstick (stored in the fixture: 1.36e-07,
      1.54e-07), floor 1e-6.  Both are evaluations of one formula that differ in summation order; the factor is headroom for the separable form.
      The tests print every measured distance before they assert; no GPU run is recorded yet (DESIGN 4.11 says so).
Run this file as the GPU suite does: under `timeout`, with -x, so that the run ends at the first fault."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metrics64 as m64
from conftest import GOLD
from test_metrics_golden import SEGM, SSIM_PAIRS, check_summary, segm_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mgold():
    return np.load(os.path.join(GOLD, "metrics.npz"))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ssim_bound(mgold):
    return np.maximum(4.0 * mgold["ssim:dev"], 1e-6)


# ---------------------------------------------------------------- segmentation
@pytest.mark.parametrize("name", SEGM)
def test_segm_fixture_cases(mgold, name):
    from nvfi_amd.utils import metric_segm as ms
    c = segm_case(mgold, name)
    B, N, K = c["mask"].shape
    G = c["counts"].shape[1]
    mask, segm = _cuda(c["mask"]), _cuda(c["segm"])
    for n_gt in (G, None):
        counts, conf, bad, pred = ms.segm_confusion(mask, segm, n_gt, want_pred=True)
        hc, hs = ms.confusion_to_host(counts, conf, bad)
        for b in range(B):
            yc, ys, yp, _ = m64.confusion64(c["mask"][b], c["segm"][b], hc.shape[1])
            assert np.array_equal(hc[b], yc) and np.array_equal(pred[b].cpu().numpy(), yp)
            e = np.max(np.abs(hs[b] - ys) / np.maximum(np.abs(ys), 1e-300))
            print(f"[metrics] {name}[{b}] G={hc.shape[1]}: conf_sum relative distance from the yardstick {e:.2e}")
            assert e <= 1e-12
    ev = ms.SegmEvaluator(K, keep_labels=True)
    for b in range(B):
        ev.update(mask[b], segm[b])
    s = ev.summary(int(c["thresh"]), aligned=True)
    check_summary(s, c, name)
    assert np.array_equal(torch.stack(s["aligned"]).cpu().numpy().reshape(-1), c["aligned"])
    # the reference's own entry points on device tensors
    iou, matched, conf, n_gt = ms.accumulate_eval_results(segm.float(), mask, int(c["thresh"]))
    assert np.array_equal(matched, c["Pred_Matched"]) and n_gt == int(c["N_GT_Inst"])
    np.testing.assert_allclose(iou, c["Pred_IoU"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(conf, c["Confidence"], rtol=4 * float(mgold["segm:conf_dev"]), atol=0)
    cm = ms.ClusteringMetrics()(mask, segm.long(), int(c["thresh"]))
    np.testing.assert_allclose(np.array(cm["iou"], np.float64), c["iou"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(cm["ri"], c["ri"], rtol=1e-12, atol=0)


def _frame(rng, B, N, K, G, coherent=True):
    z = rng.standard_normal((B, N, K)).astype(np.float32)
    mask = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    mask = mask.astype(np.float32)
    mask[:, ::7] = 0.0                                      # all-zero rows -> 0
    mask[:, 3::11, K - 1] = mask[:, 3::11].max(-1)          # exact ties with the last class -> the lower index
    segm = (np.arange(N)[None, :] * G // max(N, 1) + np.arange(B)[:, None]) % G if coherent else rng.integers(0, G, (B, N))
    return mask, segm.astype(np.int32)


@pytest.mark.parametrize("N", [1, 63, 65, 1000, 4097])
def test_segm_ragged_sizes(N):
    from nvfi_amd.utils import metric_segm as ms
    rng = np.random.default_rng(N)
    for B, K, G, coherent in ((1, 8, 8, True), (5, 3, 2, False), (1, 5, 32, False), (5, 12, 7, True), (1, 32, 32, False), (1, 1, 1, True)):
        mask, segm = _frame(rng, B, N, K, G, coherent)
        counts, conf, bad, pred = ms.segm_confusion(_cuda(mask), _cuda(segm), G, want_pred=True)
        hc, hs = ms.confusion_to_host(counts, conf, bad)
        for b in range(B):
            yc, ys, yp, _ = m64.confusion64(mask[b], segm[b], G)
            assert np.array_equal(hc[b], yc) and np.array_equal(pred[b].cpu().numpy(), yp), (N, B, K, G)
            np.testing.assert_allclose(hs[b], ys, rtol=1e-12, atol=0)
        assert hc.sum() == B * N


def test_segm_full_frame_and_repeats():
    """an 800 x 800 x 8 mask map: exact counts, and every output bit-identical over repeated calls"""
    from nvfi_amd.utils import metric_segm as ms
    rng = np.random.default_rng(800)
    H = W = 800
    y, x = np.mgrid[0:H, 0:W]
    segm = ((y // 160) * 2 + (x // 400)).astype(np.int32) % 8
    z = rng.standard_normal((H * W, 8)).astype(np.float32)
    z[np.arange(H * W), (segm.reshape(-1) + (rng.random(H * W) < 0.1)) % 8] += 3.0
    mask = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
    mask[(y < 40).reshape(-1)] = 0.0
    tm, ts = _cuda(mask)[None], _cuda(segm.reshape(1, -1))
    first = ms.segm_confusion(tm, ts, 8, want_pred=True)
    yc, ys, yp, _ = m64.confusion64(mask, segm.reshape(-1), 8, loops=False)
    hc, hs = ms.confusion_to_host(*first[:3])
    assert np.array_equal(hc[0], yc) and np.array_equal(first[3][0].cpu().numpy(), yp)
    np.testing.assert_allclose(hs[0], ys, rtol=1e-12, atol=0)
    for _ in range(3):
        again = ms.segm_confusion(tm, ts, 8, want_pred=True)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    # the call returns while the stream is still busy with earlier work: it does not wait for the device
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)
    ev = ms.SegmEvaluator(8, 8)
    ev.update(tm[0].reshape(H, W, 8), ts[0].reshape(H, W))
    assert not torch.cuda.current_stream().query(), "SegmEvaluator.update waited for the device"
    s = ev.summary()
    assert s["N_GT_Inst"] == 8 and 0.0 < float(s["RI"]) <= 1.0


def test_out_of_range_label_is_reported_and_writes_nothing_outside():
    """labels outside [0, G): counted in bad_labels, counted nowhere else, and - with guard words around every output - nothing outside the
    outputs is touched.  (The labels are only ever compared, never used as an address before the range check.)"""
    from nvfi_amd import _lib
    from nvfi_amd.utils import metric_segm as ms
    rng = np.random.default_rng(9)
    B, N, K, G = 2, 3000, 8, 4
    mask, segm = _frame(rng, B, N, K, G)
    wrong = rng.choice(N, 37, replace=False)
    segm[1, wrong[:20]] = G                  # just outside
    segm[1, wrong[20:30]] = -1
    segm[1, wrong[30:]] = 2 ** 31 - 1
    tm, ts = _cuda(mask), _cuda(segm)
    guard = 1024
    sent64, sent32 = -0x0123456789ABCDE, 0x5A5A5A5
    cbuf = torch.full((2 * guard + B * G * K,), sent64, dtype=torch.int64, device="cuda")
    fbuf = torch.full((2 * guard + B * K,), -7.25, dtype=torch.float64, device="cuda")
    bbuf = torch.full((2 * guard + B,), sent32, dtype=torch.int32, device="cuda")
    pbuf = torch.full((2 * guard + B * N,), sent32, dtype=torch.int32, device="cuda")
    counts, conf, bad, pred = cbuf[guard:-guard], fbuf[guard:-guard], bbuf[guard:-guard], pbuf[guard:-guard]
    lib = _lib.lib()
    nbytes = C.c_int64(0)
    _lib.check(lib.nvfi_metrics_workspace_bytes(1, B, K, 0, 0, C.byref(nbytes)))
    ws = torch.full((int(nbytes.value) + 2 * guard,), 0x77, dtype=torch.uint8, device="cuda")
    wsp = C.c_void_p(ws.data_ptr() + guard)
    assert (ws.data_ptr() + guard) % 256 == 0
    _lib.check(lib.nvfi_segm_confusion(B, N, K, G, _lib.ptr(tm), _lib.ptr(ts), _lib.ptr(counts), _lib.ptr(conf), _lib.ptr(pred), _lib.ptr(bad),
                                       wsp, int(nbytes.value), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for buf, s in ((cbuf, sent64), (fbuf, -7.25), (bbuf, sent32), (pbuf, sent32)):
        assert bool((buf[:guard] == s).all()) and bool((buf[-guard:] == s).all())
    assert bool((ws[:guard] == 0x77).all()) and bool((ws[-guard:] == 0x77).all())
    assert bad.cpu().tolist() == [0, 37]
    hc = counts.reshape(B, G, K).cpu().numpy()
    for b in range(B):
        yc, ys, yp, nbad = m64.confusion64(mask[b], segm[b], G)
        assert np.array_equal(hc[b], yc) and nbad == (0, 37)[b] and hc[b].sum() == N - nbad
        assert np.array_equal(pred.reshape(B, N)[b].cpu().numpy(), yp)
        np.testing.assert_allclose(conf.reshape(B, K)[b].cpu().numpy(), ys, rtol=1e-12, atol=0)
    with pytest.raises(_lib.NvfiError, match="outside"):
        ms.accumulate_eval_results(ts, tm)
    ev = ms.SegmEvaluator(K, G)
    ev.update(tm[1], ts[1])                 # queued without complaint: the check is deferred to the read
    with pytest.raises(_lib.NvfiError, match="37"):
        ev.summary()


# ---------------------------------------------------------------- SSIM
@pytest.mark.parametrize("name", SSIM_PAIRS)
def test_ssim_fixture_pairs(mgold, name):
    from nvfi_amd.utils import metrics
    p, g = mgold[f"ssim:{name}:pred"], mgold[f"ssim:{name}:gt"]
    y = np.array(m64.ssim64(p, g, mgold["ssim:window2d"]))
    tp, tg = _cuda(p)[None], _cuda(g)[None]
    st = metrics.ssim_stats(tp, tg)
    d = np.abs(st[0].cpu().numpy() - y)
    bound = ssim_bound(mgold)
    print(f"[metrics] {name}: ssim / cs distance from the float64 yardstick {d[0]:.2e} / {d[1]:.2e}, bound {bound[0]:.2e} / {bound[1]:.2e}")
    assert (d <= bound).all()
    # channel-last storage read in place: the same bits
    hwc = tp.permute(0, 2, 3, 1).contiguous(), tg.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(metrics.ssim_stats(*hwc, layout="BHWC"), st)
    assert torch.equal(metrics.ssim_frames(hwc[0][0], hwc[1][0]), st[:, 0])
    assert torch.equal(metrics.ssim_stats(hwc[0].permute(0, 3, 1, 2), hwc[1].permute(0, 3, 1, 2)), st)      # a permuted VIEW as (B, C, H, W)
    # the reference's call: fp32 results, the golden within its own error + ours
    s, cs = metrics.SSIM()(tp, tg, full=True)
    assert s.dtype == torch.float32 and s.dim() == 0
    assert abs(float(s) - mgold[f"ssim:{name}:ref"][0]) <= bound[0] + mgold["ssim:dev"][0] + 1e-7
    assert abs(float(cs) - mgold[f"ssim:{name}:ref"][1]) <= bound[1] + mgold["ssim:dev"][1] + 1e-7
    # the derived range equals the given one, and repeated calls are bit-identical
    assert torch.equal(metrics.ssim_stats(tp, tg, L=float(mgold[f"ssim:{name}:L"])), st)
    for _ in range(3):
        assert torch.equal(metrics.ssim_stats(tp, tg), st)


def _images(rng, B, Cc, H, W, scale=1.0):
    g = rng.random((B, Cc, H, W))
    g = 0.5 * g + 0.5 * np.roll(g, 1, -1)
    p = np.clip(g + 0.07 * rng.standard_normal(g.shape), 0, 1)
    return (scale * p).astype(np.float32), (scale * g).astype(np.float32)


@pytest.mark.parametrize("H,W", [(11, 11), (12, 43), (27, 33), (42, 26), (43, 27), (75, 50)])
def test_ssim_ragged_sizes(mgold, H, W):
    from nvfi_amd.utils import metrics
    rng = np.random.default_rng(H * 100 + W)
    bound = ssim_bound(mgold)
    for B, Cc in ((1, 3), (5, 1), (5, 4)):
        p, g = _images(rng, B, Cc, H, W)
        st = metrics.ssim_stats(_cuda(p), _cuda(g)).cpu().numpy()
        for b in range(B):
            d = np.abs(st[b] - np.array(m64.ssim64(p[b], g[b], mgold["ssim:window2d"])))
            assert (d <= bound).all(), (H, W, B, Cc, b, d)
        s = metrics.SSIM()(_cuda(p), _cuda(g), size_average=False)
        assert s.shape == (B,) and np.allclose(s.cpu().numpy(), st[:, 0], rtol=0, atol=1e-7)


def test_ssim_derived_range_rule(mgold):
    """max(pred) > 128 -> 255, min(pred) < -0.5 -> min_val -1: over the whole call for SSIM(), per image for estim_error / ssim_frames"""
    from nvfi_amd.utils import metrics
    rng = np.random.default_rng(1)
    p, g = _images(rng, 3, 3, 30, 31)
    p[1] *= 255.0; g[1] *= 255.0            # one byte-range image in the batch
    p[2] = 2 * p[2] - 1; g[2] = 2 * g[2] - 1
    tp, tg = _cuda(p), _cuda(g)
    w = mgold["ssim:window2d"]
    whole = metrics.ssim_stats(tp, tg).cpu().numpy()                        # L = 255 - (-1) = 256 for every image
    each = metrics.ssim_stats(tp, tg, per_image_range=True).cpu().numpy()   # L = 1, 255, 2
    bound = ssim_bound(mgold)
    for b, L in enumerate((1, 255, 2)):
        assert m64.derived_range(p[b]) == L
        assert (np.abs(each[b] - np.array(m64.ssim64(p[b], g[b], w))) <= bound).all()
        assert (np.abs(whole[b] - np.array(m64.ssim64(p[b], g[b], w, L=256))) <= bound).all()
    assert abs(metrics.estim_error(tp[:1], tg[:1])["ssim"] - each[0, 0]) == 0.0


def test_ssim_full_frame(mgold):
    from nvfi_amd.utils import metrics
    rng = np.random.default_rng(2)
    p, g = _images(rng, 1, 3, 800, 800)
    hp, hg = _cuda(p[0].transpose(1, 2, 0)), _cuda(g[0].transpose(1, 2, 0))          # (H, W, 3), as the renderer returns a frame
    s = metrics.ssim_frames(hp, hg)
    y = m64.ssim64(p[0], g[0], mgold["ssim:window2d"])
    d = abs(float(s[0]) - y[0])
    print(f"[metrics] 800 x 800 x 3 frame: ssim distance from the float64 yardstick {d:.2e}")
    assert d <= ssim_bound(mgold)[0]
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)
    s2 = metrics.ssim_frames(hp, hg)
    assert not torch.cuda.current_stream().query(), "ssim_frames waited for the device"
    assert torch.equal(s, s2)


# ---------------------------------------------------------------- end to end
def _scene():
    from helpers import make_model
    from nvfi_amd.models import MaskField, Renderer
    gold = np.load(os.path.join(GOLD, "hotpath.npz"))
    model, meta = make_model("A")
    model.nvfi.alphaMask = None
    mf = MaskField(n_layer=4, n_dim=128, skips=[], mask_dim=8).cuda()
    mf.load_state_dict({k[len("A:mask:sd:"):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("A:mask:sd:")})
    H, W, focal = 28, 36, 34.0
    aabb = np.asarray(meta["aabb"], np.float32).reshape(2, 3)
    poses, times = [], []
    for th, t in ((20.0, 0.30), (75.0, 19 / 60.0), (140.0, 0.45)):
        c, s = np.cos(np.deg2rad(th)), np.sin(np.deg2rad(th))
        R_ = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = R_
        pose[:3, 3] = R_ @ np.array([0, 0, 4.0], np.float32) + (aabb[0] + aabb[1]) * 0.5
        poses.append(pose); times.append(t)
    return model, meta, mf, Renderer(model, 0, 0, 2048), poses, times, H, W, focal


def test_render_segm_evaluation_end_to_end(tmp_path):
    """the loop of test_segm_render.py on the small synthetic field + MaskField of the mask-branch tests: its summary is stage 2 applied to the
    yardstick's confusion of the very mask maps it rendered"""
    from nvfi_amd.utils import metric_segm as ms
    from nvfi_amd.utils import render_segm_evaluation
    model, meta, mf, ren, poses, times, H, W, focal = _scene()
    y, x = np.mgrid[0:H, 0:W]
    gt = [((y // 10 + (x + 5 * i) // 12) % 4).astype(np.int64) for i in range(len(poses))]
    res = render_segm_evaluation(model, ren, mf, poses, times, gt, H, W, focal, float(meta["near"]), float(meta["far"]),
                                 white_background=bool(meta["white_background"]), savedir=str(tmp_path), return_maps=True)
    assert model.nvfi.mask_field is None
    maps = [m.cpu().numpy() for m in res["segm_maps"]]
    assert all(m.shape == (H, W, 8) for m in maps)
    print("[metrics] render_segm_evaluation: largest composited mask value per frame", [round(float(m.max()), 4) for m in maps])
    yard = [m64.confusion64(m.reshape(-1, 8), g.reshape(-1), 32) for m, g in zip(maps, gt)]
    want = ms.summary_from_confusion(np.stack([v[0] for v in yard]), np.stack([v[1] for v in yard]))
    assert np.array_equal(res["Pred_Matched"], want["Pred_Matched"]) and res["N_GT_Inst"] == want["N_GT_Inst"] == 4 * len(poses)
    for k in ("AP", "PQ", "F1", "Pre", "Rec", "mIoU", "RI"):
        assert abs(float(res[k]) - float(want[k])) <= 1e-12, (k, res[k], want[k])
    np.testing.assert_allclose(res["Confidence"], want["Confidence"], rtol=1e-12, atol=0)
    print("[metrics] render_segm_evaluation:", {k: round(float(res[k]), 6) for k in ("AP", "PQ", "F1", "Pre", "Rec", "mIoU", "RI")})
    assert len(res["aligned"]) == len(poses) and res["aligned"][0].shape == (H, W)
    assert sorted(os.listdir(tmp_path)) in (["r_%03d_segm_vis.png" % i for i in range(len(poses))], ["segm_labels.npy"])      # (without PIL: the raw labels)


def test_estim_error_and_eval_driver_ssim(mgold):
    from nvfi_amd.utils import estim_error, mse2psnr, render_test_evaluation
    model, meta, mf, ren, poses, times, H, W, focal = _scene()
    near, far, wb = float(meta["near"]), float(meta["far"]), bool(meta["white_background"])
    base = render_test_evaluation(model, ren, poses, times, None, H, W, focal, near, far, white_background=wb, update_alpha_mask=False)
    frames = base["images"].astype(np.float32) / 255.0
    rng = np.random.default_rng(4)
    targets = np.clip(frames + 0.05 * rng.standard_normal(frames.shape), 0, 1).astype(np.float32)
    plain = render_test_evaluation(model, ren, poses, times, targets, H, W, focal, near, far, white_background=wb, update_alpha_mask=False)
    assert set(plain) == {"psnr", "mean_psnr", "images"}                   # off by default: the return value is what it was
    res = render_test_evaluation(model, ren, poses, times, targets, H, W, focal, near, far, white_background=wb, update_alpha_mask=False, with_ssim=True)
    assert res["psnr"] == plain["psnr"] and np.array_equal(res["images"], plain["images"]) and len(res["ssim"]) == len(poses)
    assert 0.0 < res["mean_ssim"] < 1.0
    est = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)               # (B, C, H, W) views of channel-last frames
    tgt = torch.from_numpy(targets).cuda().permute(0, 3, 1, 2)
    err = estim_error(est, tgt)
    assert set(err) == {"mse", "psnr", "ssim"} or set(err) == {"mse", "psnr", "ssim", "lpips"}
    assert abs(err["psnr"] - mse2psnr(err["mse"])) <= 1e-5 * abs(err["psnr"])      # fp32 log10 of an fp32 mean
    want = np.mean([m64.ssim64(frames[i].transpose(2, 0, 1), targets[i].transpose(2, 0, 1), mgold["ssim:window2d"])[0] for i in range(len(poses))])
    assert abs(err["ssim"] - want) <= ssim_bound(mgold)[0]
