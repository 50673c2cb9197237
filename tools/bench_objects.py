#!/usr/bin/env python
"""One 800 x 800 test-mode frame of the bench scene (bench.build_scene, bench camera) at t = 19/60 with a K = 8 MaskField attached, timed four ways:
  mask     Renderer.render(mode="test"): the frame + the mask branch (mask_map), what a user had before;
  layers   Renderer.render_objects: the same + obj_rgb, obj_acc, obj_depth (one nvfi_render_objects per chunk behind the mask branch);
  public   the layer maps assembled from the calls a user had before: per chunk nvfi_render_fwd, the masked count read on the host,
           nvfi_render_export_masked for the masked samples' warped positions and indices, MaskField on them, torch index_add.  The per-sample
           COLOURS never leave the workspace, so this assembly cannot build obj_rgb at all: it is timed for what it can build, obj_acc and
           obj_depth.  Kept here, not in the package;
  select   Renderer.render_objects(select=...) with one object removed: the frame re-rendered with the MaskField over all valid samples.
Expectation from counting (nothing here has been measured before): the select pass costs V (3 128 + 3 128^2 + 128 K) multiply-adds per chunk, V the
valid samples - about three times the mask branch's M of them; the layer kernel reads M (32 + 4 + 2) floats once.  The JSON line carries V and M of
the last chunk (last_counters) beside the times.
HIP events, the median of --reps runs, the steps alternating round by round inside one child process per step set under its own time limit.
    python tools/bench_objects.py [--out profiles/objects_timing.json] [--reps 5]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, K = 19.0 / 60.0, 8
LIMIT = 540       # seconds


def scene():
    import numpy as np
    import torch
    import bench
    from nvfi_amd.models import Camera, MaskField, Renderer
    dev = torch.device("cuda", 0)
    model = bench.build_scene(dev)
    model.eval()
    torch.manual_seed(7)
    mf = MaskField(n_layer=4, n_dim=128, input_dim=3, skips=[], mask_dim=K, mask_act="softmax").to(dev).eval()
    with torch.no_grad():
        mf.mask_fc.weight.mul_(100.0)          # peaked masks, as a trained decomposition has them
    model.nvfi.mask_field = mf
    focal = 0.5 * bench.W_IMG / np.tan(0.5 * bench.ANGLE_X)
    cam = Camera(bench.pose_spherical(30.0, -30.0, 4.0).to(dev), bench.H_IMG, bench.W_IMG, focal, None, 1.0, 8.0)
    return model, Renderer(model, 0, 0, 2048), cam, dev


def public_maps(f, rays, chunk=32768):
    """obj_acc and obj_depth out of the public calls a user had before, chunk by chunk (obj_rgb cannot be built: no per-sample colours)"""
    import ctypes as C
    import torch
    from nvfi_amd import _lib
    from nvfi_amd.models.tensorf_keyframe import _stream_ptr
    L = _lib.lib()
    o_all, d_all = rays.ray_origins.reshape(-1, 3).contiguous().float(), rays.ray_directions.reshape(-1, 3).contiguous().float()
    dev = o_all.device
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
        xw = torch.empty(M, 3, device=dev)
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        if M:
            _lib.check(L.nvfi_render_export_masked(C.byref(desc), R, T, flags, _lib.ptr(ws), ws.numel(),
                                                   M, _lib.ptr(xw), _lib.ptr(idx), _stream_ptr()))
        ray, smp = idx // S, idx % S
        inside = bool(((f.aabb[0] <= o) & (o <= f.aabb[1])).any())
        if inside:
            tmin = torch.full_like(o[:, 0], f.near_far[0])
        else:
            vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
            tmin = torch.minimum((f.aabb[1] - o) / vec, (f.aabb[0] - o) / vec).amax(-1).clamp(f.near_far[0], f.near_far[1])
        z = tmin[ray] + f._step_host * smp.float()
        wm = w.reshape(-1)[idx][:, None] * f.mask_field(xw)
        outs.append((torch.zeros(R, K, device=dev).index_add(0, ray, wm), torch.zeros(R, K, device=dev).index_add(0, ray, wm * z[:, None])))
    return [torch.cat(x, 0) for x in zip(*outs)]


def child(reps):
    import torch
    model, ren, cam, dev = scene()
    f = model.nvfi
    rays = cam.rays.to(dev)
    sel = [1.0] * K
    fns = {"mask": lambda: ren.render(T, rays, white_background=True, mode="test"),
           "layers": lambda: ren.render_objects(T, rays, white_background=True),
           "public": lambda: public_maps(f, rays),
           "select": lambda: ren.render_objects(T, rays, select=sel, white_background=True)}
    ms = {k: [] for k in fns}
    res = {}
    with torch.no_grad():
        full = fns["layers"]()
        sel[int(full[6].reshape(-1, K).sum(0).argmax())] = 0.0        # remove the dominant object
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):                 # alternating: one run of every step per round
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
                if k in ("layers", "select"):
                    cnt = f.last_counters.cpu().tolist()
                    res[k + "_last_chunk"] = dict(valid=cnt[0], masked=cnt[2])
                if k == "public":
                    res["public_vs_layers_obj_acc"] = float((out[0] - full[6].reshape(-1, K)).abs().max())
    for k, v in ms.items():
        res[k] = dict(ms=sorted(v)[len(v) // 2], ms_all=v)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                       capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
        sys.exit(1)
    res = {"t": T, "K": K, "frame": [800, 800]}
    res.update(json.loads(line[0][7:]))
    res["layers_minus_mask_ms"] = res["layers"]["ms"] - res["mask"]["ms"]
    res["select_minus_layers_ms"] = res["select"]["ms"] - res["layers"]["ms"]
    out = json.dumps(res)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
