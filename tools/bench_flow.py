#!/usr/bin/env python
"""One 800 x 800 test-mode frame of the bench scene (bench.build_scene, bench camera) at t = 19/60 with dt = 1/60, timed three ways:
  render  Renderer.render(mode="test"): the frame alone;
  flow    Renderer.render_flow: the frame + vel_map, flow_map, flow2d (one nvfi_render_fwd + one nvfi_render_flow per chunk);
  public  the same three maps assembled from the calls a user had before: per chunk nvfi_render_fwd, the masked count read on the host,
          nvfi_render_export_masked for the list of masked samples (it exports the warped keyframe positions, so the un-warped positions at t
          are rebuilt by hand in torch), field.vel / field.integrate_pos on them, index_add.  Kept here, not in the package.
Expectation from counting (nothing here has been measured before): the branch costs about M (1 + 2 steps) net evaluations against the warp's
N 2 steps, so `flow - render` should stay under the frame's own warp time when M < N; the JSON line carries N and M (last_counters) beside the
times so that the reader can check.
Each step runs in a child process of its own under its own time limit, one after the other; the first failure stops the tool.
    python tools/bench_flow.py [--out profiles/flow_timing.json] [--reps 5]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, DT = 19.0 / 60.0, 1.0 / 60.0
STEPS = {"render": 240, "flow": 240, "public": 420}       # seconds


def scene():
    import torch
    import bench
    from nvfi_amd.models import Camera, Renderer
    dev = torch.device("cuda", 0)
    model = bench.build_scene(dev)
    model.eval()
    focal = 0.5 * bench.W_IMG / __import__("numpy").tan(0.5 * bench.ANGLE_X)
    cam = Camera(bench.pose_spherical(30.0, -30.0, 4.0).to(dev), bench.H_IMG, bench.W_IMG, focal, None, 1.0, 8.0)
    return model, Renderer(model, 0, 0, 2048), cam, dev


def public_maps(f, cam, rays, chunk=32768):
    """the three maps out of the public calls a user had before, chunk by chunk"""
    import ctypes as C
    import torch
    from nvfi_amd import _lib
    from nvfi_amd.models.tensorf_keyframe import _stream_ptr
    L = _lib.lib()
    o_all, d_all = rays.ray_origins.reshape(-1, 3).contiguous().float(), rays.ray_directions.reshape(-1, 3).contiguous().float()
    dev = o_all.device
    half = (f.aabb[1] - f.aabb[0]) / 2
    pose = torch.as_tensor(cam.pose, device=dev)[:3, :4]
    desc = f._desc()
    S = desc.n_samples
    flags = _lib.NVFI_WHITE_BG
    outs = []
    for c in range(0, o_all.shape[0], chunk):
        o, d = o_all[c:c + chunk].contiguous(), d_all[c:c + chunk].contiguous()
        R = o.shape[0]
        ws = torch.empty(_lib.bytes_of(L.nvfi_render_workspace_bytes_t, C.byref(desc), R, flags, T), dtype=torch.uint8, device=dev)
        rgb, depth, acc = torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
        w = torch.empty(R, S, device=dev)
        counters = torch.empty(_lib.NCOUNTERS, dtype=torch.int64, device=dev)
        _lib.check(L.nvfi_render_fwd(C.byref(desc), R, _lib.ptr(o), _lib.ptr(d), None, T, flags, _lib.ptr(rgb),
                                     _lib.ptr(depth), _lib.ptr(acc), _lib.ptr(w), _lib.ptr(ws), ws.numel(), _lib.ptr(counters), _stream_ptr()))
        M = int(counters[2])                             # waits for the device: the masked count sizes everything below
        xw = torch.empty(M, 3, device=dev)               # (the warped keyframe positions: exported, but not what the maps need)
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        if M:
            _lib.check(L.nvfi_render_export_masked(C.byref(desc), R, T, flags, _lib.ptr(ws), ws.numel(),
                                                   M, _lib.ptr(xw), _lib.ptr(idx), _stream_ptr()))
        ray, smp = idx // S, idx % S
        # sample_ray by hand (tensorf_base.py:290-314, eval mode): the un-warped positions at time t
        inside = bool(((f.aabb[0] <= o) & (o <= f.aabb[1])).any())
        if inside:
            tmin = torch.full_like(o[:, 0], f.near_far[0])
        else:
            vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
            tmin = torch.minimum((f.aabb[1] - o) / vec, (f.aabb[0] - o) / vec).amax(-1).clamp(f.near_far[0], f.near_far[1])
        z = tmin[ray] + f._step_host * smp.float()
        x = f.normalize_coord(o[ray] + d[ray] * z[:, None])
        tt = torch.full_like(x[:, :1], T)
        v = f.vel(torch.cat([x, tt], -1))
        xd = f.integrate_pos(x, tt, tt + DT)
        wm = w.reshape(-1)[idx][:, None]

        def pix(xn):
            q = (f.aabb[0] + (xn + 1) * half - pose[:, 3]) @ pose[:, :3]
            return torch.stack([cam.focal * q[:, 0] / -q[:, 2], -(cam.focal * q[:, 1] / -q[:, 2])], 1)

        outs.append((torch.zeros(R, 3, device=dev).index_add(0, ray, wm * half * v),
                     torch.zeros(R, 3, device=dev).index_add(0, ray, wm * half * (xd - x)),
                     torch.zeros(R, 2, device=dev).index_add(0, ray, wm * (pix(xd) - pix(x)))))
    return [torch.cat(x, 0) for x in zip(*outs)]


def child(step, reps):
    import torch
    model, ren, cam, dev = scene()
    f = model.nvfi
    rays = cam.rays.to(dev)
    fn = {"render": lambda: ren.render(T, rays, white_background=True, mode="test"),
          "flow": lambda: ren.render_flow(T, rays, DT, camera=cam, white_background=True),
          "public": lambda: public_maps(f, cam, rays)}[step]
    with torch.no_grad():
        out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    res = dict(step=step, ms=sorted(ms)[len(ms) // 2], ms_all=ms)
    if step != "public":
        cnt = f.last_counters.cpu().tolist()
        res.update(last_chunk_valid=cnt[0], last_chunk_warped=cnt[1], last_chunk_masked=cnt[2])
    if step == "flow":
        res.update(max_abs=[float(out[i].abs().max()) for i in (4, 5, 6)])
    if step == "public":
        res.update(max_abs=[float(x.abs().max()) for x in out])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    res = {"t": T, "dt": DT, "frame": [800, 800]}
    for step, limit in STEPS.items():
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps)],
                           capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {step} failed (exit {r.returncode}) after {time.time() - t0:.0f} s; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            sys.exit(1)
        res[step] = json.loads(line[0][7:])
    res["flow_minus_render_ms"] = res["flow"]["ms"] - res["render"]["ms"]
    out = json.dumps(res)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
