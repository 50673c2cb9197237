"""Renderer: ray chunk loop + reshape to rays.restore_shape (reference models/renderer.py:7-65)."""
import os

import torch
import torch.nn as nn

# read once.  NVFI_EVAL_CHUNK: upper bound of the internal test-mode chunk (rays); NVFI_EVAL_STREAMS: 1 = the reference's plain
# loop on the current stream; NVFI_EVAL_WS_BYTES: byte budget for the chunks in flight (workspace + the (R, S) weights output of each)
_EVAL_CHUNK_MAX = int(os.environ.get("NVFI_EVAL_CHUNK", "32768"))
_EVAL_STREAMS = 1 if os.environ.get("NVFI_EVAL_STREAMS", "2") == "1" else 2
_EVAL_WS_BYTES = int(float(os.environ.get("NVFI_EVAL_WS_BYTES", str(8 << 30))))


class Renderer(nn.Module):
    def __init__(self, tensorf, batch_size, test_batch_size, ray_chunk, distance_scale=1, lindisp=False,
                 perturb=True, tensorf_sample=True, ndc=False):
        super().__init__()
        self.tensorf = tensorf
        self.batch_size, self.test_batch_size = batch_size, test_batch_size
        self.lindisp, self.perturb, self.distance_scale = lindisp, perturb, distance_scale
        self.tensorf_sample, self.ndc, self.ray_chunk = tensorf_sample, ndc, ray_chunk
        self.eval_chunk = None          # None: derived from the byte budget below; an int pins the internal test-mode chunk (rays)
        self.eval_ws_bytes = _EVAL_WS_BYTES

    def _eval_chunk(self, t, transfer_vel, flow=False, objects=False):
        """Internal chunk of a test-mode frame: the largest multiple of the caller's ray_chunk, at most NVFI_EVAL_CHUNK, whose in-flight
        memory - _EVAL_STREAMS x (nvfi_render_workspace_bytes_t + the (R, S) weights) - stays inside `eval_ws_bytes` (8 GiB by default; the
        workspace and weights grow with nSamples, ~1000 after the last upsampling).  A caller who lowered ray_chunk to bound memory keeps that
        bound by lowering eval_ws_bytes (or pinning eval_chunk): the chunk never drops below ray_chunk, which is the reference's loop."""
        base = max(1, int(self.ray_chunk))
        if self.eval_chunk is not None:
            return max(1, int(self.eval_chunk))
        field = getattr(self.tensorf, "nvfi", None)
        if field is None or not hasattr(field, "render_workspace_bytes"):
            return base
        key = (base, int(field.nSamples), self.eval_ws_bytes, bool(transfer_vel), float(t), bool(flow), bool(objects))
        c = self.__dict__.get("_eval_chunk_cache")
        if c is not None and c[0] == key:
            return c[1]
        chunk = max(base, _EVAL_CHUNK_MAX // base * base)
        while chunk > base:
            # (flow: the larger workspace nvfi_render_flow plans, and three more small maps per ray)
            ws = field.render_workspace_bytes(chunk, t, transfer=transfer_vel, flow=True) if flow else field.render_workspace_bytes(chunk, t, transfer=transfer_vel)
            need = _EVAL_STREAMS * (ws + chunk * (int(field.nSamples) + (16 if flow else 8)) * 4)
            if objects:
                # (objects: the workspace with the mask branch's and the select pass's room, and 6 K more floats per ray: mask_map + the layers)
                k = int(getattr(getattr(field, "mask_field", None), "mask_dim", 32))
                ws = field.render_workspace_bytes(chunk, t, transfer=transfer_vel, objects=True)
                need = _EVAL_STREAMS * (ws + chunk * (int(field.nSamples) + 8 + 6 * k) * 4)
            if need <= self.eval_ws_bytes:
                break
            chunk = max(base, (chunk // 2) // base * base)
        self.__dict__["_eval_chunk_cache"] = (key, chunk)
        return chunk

    def forward(self, t, rays, white_background=False, transfer_vel=False):
        return self._chunks(t, rays, white_background, transfer_vel, None)

    def render_flow(self, t, rays, dt, camera=None, white_background=False, transfer_vel=False):
        """Test-mode render of a frame with the velocity field's maps (NVFi.render_ray_flow; the reference has no counterpart) -> rgb, depth,
        acc, weights, vel_map (..., 3), flow_map (..., 3), flow2d (..., 2) or None without a camera, reshaped to rays.restore_shape.  Same
        byte-budgeted chunks and side streams as a test-mode `forward`; the chunks are independent, so the result does not depend on them.  A model in training mode is
        switched to eval mode and stays there, as after `render(mode="test")`: the caller calls `train()` again before the next step."""
        if self.tensorf.training:
            self.tensorf.eval()
        with torch.no_grad():
            return self._chunks(t, rays, white_background, transfer_vel, (float(dt), camera))

    def render_objects(self, t, rays, select=None, white_background=False, transfer_vel=False):
        """Test-mode render of a frame with the per-object layers of the field's mask_field (NVFi.render_ray_objects; the reference has no
        counterpart) -> rgb, depth, acc, weights, mask_map (..., K), obj_rgb (..., K, 3), obj_acc (..., K), obj_depth (..., K), reshaped to
        rays.restore_shape.  `select` as in TensorVMKeyframeTimeKplane.render_objects: None, K factors in [0, 1], or integer indices of the
        objects to keep - the scene is re-rendered without the others, occlusion recomputed.  Same byte-budgeted chunks (the new room counted) and
        side streams as a test-mode `forward`; the chunks are independent.  A model in training mode is switched to eval mode and stays there."""
        if self.tensorf.training:
            self.tensorf.eval()
        with torch.no_grad():
            return self._chunks(t, rays, white_background, transfer_vel, None, objects=(select,))

    def _chunks(self, t, rays, white_background, transfer_vel, flow, objects=None):
        ray_o = rays.ray_origins.reshape(-1, 3)
        ray_d = rays.ray_directions.reshape(-1, 3)
        n_all = ray_o.shape[0]
        outs = [[] for _ in range(8 if objects is not None else 5 if flow is None else 7)]
        chunk = self.ray_chunk
        if objects is not None:
            chunk = self._eval_chunk(t, transfer_vel, objects=True)
        elif flow is not None:
            chunk = self._eval_chunk(t, transfer_vel, flow=True)
        elif ray_o.is_cuda and not torch.is_grad_enabled() and not self.tensorf.training:
            # test-mode rays carry no jitter and are independent (tests/test_gpu_edges.py: every prefix of a render equals the render), so the
            # reference's ray_chunk - a memory bound for its (R, S, .) torch intermediates - need not be the launch granularity here: a frame
            # goes through in pieces of up to NVFI_EVAL_CHUNK rays (default 32768: 16 MB of weights at 128 samples per ray; bounded by a byte
            # budget, _eval_chunk), 16x fewer launches
            chunk = self._eval_chunk(t, transfer_vel)
        n_chunks = n_all // chunk + int(n_all % chunk > 0)
        fn = self.tensorf.render_ray_transfer if transfer_vel else self.tensorf.render_ray
        if flow is not None:
            def fn(t_, r_o, r_d, white_bg, ndc):
                return self.tensorf.render_ray_flow(t_, r_o, r_d, flow[0], camera=flow[1], white_bg=white_bg, transfer_vel=transfer_vel)
        if objects is not None:
            field = getattr(self.tensorf, "nvfi", None)
            if objects[0] is not None and getattr(field, "mask_field", None) is not None:
                objects = (field._select_vector(objects[0], ray_o.device),)     # once per frame, before the side streams fork

            def fn(t_, r_o, r_d, white_bg, ndc):
                return self.tensorf.render_ray_objects(t_, r_o, r_d, select=objects[0], white_bg=white_bg, transfer_vel=transfer_vel)
        # a test-mode frame is some hundred independent chunks: issued alternately on two side streams, one chunk's velocity warp (matrix pipe)
        # runs beside the other's plane gathers (HBM) - every chunk call owns its workspace and outputs, nothing is shared but the weights.
        # NVFI_EVAL_STREAMS=1: the reference's plain loop on the current stream
        side = None
        if n_chunks >= 4 and ray_o.is_cuda and not torch.is_grad_enabled() and _EVAL_STREAMS != 1:
            side = self.__dict__.get("_eval_streams")
            if side is None or side[0].device != ray_o.device:
                side = self.__dict__["_eval_streams"] = [torch.cuda.Stream(device=ray_o.device) for _ in range(2)]
            main = torch.cuda.current_stream(ray_o.device)
            for s_ in side:
                s_.wait_stream(main)
        for c in range(n_chunks):
            r_o = ray_o[c * chunk:(c + 1) * chunk]
            r_d = ray_d[c * chunk:(c + 1) * chunk]
            if side is None:
                res = fn(t, r_o, r_d, white_background, self.ndc)
            else:
                with torch.cuda.stream(side[c & 1]):
                    res = fn(t, r_o, r_d, white_background, self.ndc)
                for v in res:
                    if torch.is_tensor(v):
                        v.record_stream(main)          # allocated on the side stream, consumed (torch.cat below, the caller) on the current one
            for lst, v in zip(outs, res):
                lst.append(v)
        if side is not None:
            for s_ in side:
                main.wait_stream(s_)
        # (one chunk - every training batch - needs no concatenation: five copy launches less per render)
        shp = tuple(rays.restore_shape)
        if objects is not None:
            res = [o[0] if len(o) == 1 else torch.cat(o, 0) for o in outs]
            k = res[4].shape[-1]
            return (res[0].reshape(*shp, 3), res[1].reshape(*shp), res[2].reshape(*shp), res[3].reshape(*shp, -1), res[4].reshape(*shp, k),
                    res[5].reshape(*shp, k, 3), res[6].reshape(*shp, k), res[7].reshape(*shp, k))
        if flow is not None:
            res = [None if o[0] is None else (o[0] if len(o) == 1 else torch.cat(o, 0)) for o in outs]
            rgb_map, depth_map, acc_map, weights = res[:4]
            return (rgb_map.reshape(*shp, 3), depth_map.reshape(*shp), acc_map.reshape(*shp), weights.reshape(*shp, -1),
                    res[4].reshape(*shp, 3), res[5].reshape(*shp, 3), None if res[6] is None else res[6].reshape(*shp, 2))
        rgb_map, depth_map, acc_map, weights, extra = [o[0] if len(o) == 1 else torch.cat(o, 0) for o in outs]
        return (rgb_map.reshape(*shp, 3), depth_map.reshape(*shp), acc_map.reshape(*shp),
                weights.reshape(*shp, -1), extra.reshape(*shp, extra.shape[-1]))

    def render(self, t, rays, white_background=False, mode="train", transfer_vel=False):
        if mode == "train":
            if not self.tensorf.training:     # (the reference calls .train()/.eval() unconditionally; the recursion is pure host cost)
                self.tensorf.train()
            return self.forward(t, rays, white_background)
        if self.tensorf.training:
            self.tensorf.eval()
        with torch.no_grad():
            return self.forward(t, rays, white_background, transfer_vel=transfer_vel)
