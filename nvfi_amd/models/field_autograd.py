"""The autograd boundaries of TensorVMKeyframeTimeKplane: one torch.autograd.Function per library call pair (include/nvfi_hip.h).  Each
states once how many non-tensor arguments precede its parameters (N_ARGS); the slot order of those parameters is field_slots', the flat
gradient format and the choice of the write target are field_grads'."""
import ctypes as C
import weakref

import torch

from .. import _lib
from .._lib import stream_ptr as _stream_ptr
from . import field_slots as fs
from .field_grads import _rt, _zero_grads, pack_specs, unpack_scaled


class _RenderFn(torch.autograd.Function):
    """autograd boundary around nvfi_render_fwd / nvfi_render_bwd (include/nvfi_hip.h)."""
    N_ARGS = 6      # field, t, rays_o, rays_d, jitter, flags

    @staticmethod
    def forward(ctx, field, t, rays_o, rays_d, jitter, flags, *params):
        L = _lib.lib()
        R = rays_o.shape[0]
        t_dev = getattr(t, "dev", None)        # DeviceTime: the kernels read the time from device memory; float(t) is the launch plan
        t = float(t)
        desc, ws, (rgb, depth, acc, weights, counters) = field._ray_buffers(R, rays_o.device, t, flags)      # all 8 counters are written by the call
        _lib.check(L.nvfi_render_fwd_t(C.byref(desc), R, _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(jitter),
                                       t, _lib.ptr(t_dev), flags, _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(acc),
                                       _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.ptr(counters), _stream_ptr()))
        field.last_counters = counters
        field._last_ws = ws if (flags & _lib.NVFI_WANT_MASK) else None
        field._last_call = (R, t, flags)
        if flags & _lib.NVFI_TRAIN:
            ctx.field, ctx.t, ctx.flags, ctx.ws, ctx.t_on_device = field, t, flags, ws, t_dev is not None
            ctx.vel_fp16 = int(desc.vel_fp16)      # the workspace layout depends on it: the backward plans with the forward's value
            ctx.save_for_backward(rays_o, rays_d, weights, *params)
        ctx.mark_non_differentiable(counters)
        ctx.set_materialize_grads(False)     # unused outputs (depth, acc, the R x S weights) arrive as None, not as zero tensors
        return rgb, depth, acc, weights, counters

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_weights, _gc):
        L = _lib.lib()
        rays_o, rays_d, weights, *params = ctx.saved_tensors
        field = ctx.field
        desc = field._desc(params)
        desc.vel_fp16 = ctx.vel_fp16
        need = ctx.needs_input_grad[_RenderFn.N_ARGS:]
        grads, inplace = field._grad_targets(field._render_params(), need)
        if not inplace:
            grads = _zero_grads(params, need)
        elif field.accumulate_grads_inplace == "arena":
            # library-managed in-place accumulation (the default under a plain autograd driver): see _arena_attach
            field._wait_writers()
            field._queue_join()
        G = field._grads_struct(grads)
        gs = [None if g is None else g.contiguous() for g in (g_rgb, g_depth, g_acc, g_weights)]
        R = rays_o.shape[0]
        _lib.check(L.nvfi_render_bwd_t(C.byref(desc), R, _lib.ptr(rays_o), _lib.ptr(rays_d), ctx.t, int(ctx.t_on_device),
                                     ctx.flags, _lib.ptr(weights), _lib.ptr(gs[0]), _lib.ptr(gs[1]), _lib.ptr(gs[2]),
                                     _lib.ptr(gs[3]), C.byref(G), _lib.ptr(ctx.ws), ctx.ws.numel(), _stream_ptr()))
        ctx.ws = None
        if inplace:
            return (None,) * (_RenderFn.N_ARGS + len(params))
        return (None,) * _RenderFn.N_ARGS + tuple(grads)


class _PdeFn(torch.autograd.Function):
    """nvfi_pde_loss computes the loss AND its parameter gradients in one pass; backward scales them."""
    N_ARGS = 3      # field, points, t

    @staticmethod
    def forward(ctx, field, points, t, *params):
        L = _lib.lib()
        dev = points.device
        P = points.shape[0]
        desc = field._desc()
        nbytes = _lib.bytes_of(L.nvfi_pde_workspace_bytes, C.byref(desc), P)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.zeros(4, device=dev)
        grads = _zero_grads(params)
        G = field._grads_struct_vel(grads)
        counters = torch.zeros(_lib.NCOUNTERS, dtype=torch.int64, device=dev)
        kept = torch.zeros(P, dtype=torch.uint8, device=dev) if field.pde_debug else None
        jac = torch.zeros(field.pde_debug, 6, 4, device=dev) if field.pde_debug else None
        info = (C.c_int64 * 2)()
        # split call (field.pde_split, default on): the VALUE is complete on the current stream after the Jacobian forward, the adjoint pass and
        # the weight gradients run on the field's PDE side stream - under the reference's loop, which waits for the value right after this call
        # (train_nvfi.py:233) and then differentiates the renders, the PDE adjoint overlaps with them; backward() waits for `ctx.done`
        side = field._side_stream("p") if field.pde_split else None
        _lib.check(L.nvfi_pde_loss_split(C.byref(desc), P, _lib.ptr(points), _lib.ptr(t), 1.0, _lib.ptr(out),
                                         C.byref(G), _lib.ptr(ws), ws.numel(), _lib.ptr(counters),
                                         _lib.ptr(kept), _lib.ptr(jac), int(field.pde_debug), info, _stream_ptr(),
                                         C.c_void_p(side.cuda_stream) if side is not None else None))
        ctx.done = None
        if side is not None:
            ctx.done = torch.cuda.Event()
            ctx.done.record(side)
            ws.record_stream(side)
            grads[0]._base.record_stream(side)
        field.last_pde_kept, field.last_pde_jac = kept, jac
        field.last_pde_n_kept = int(info[0])
        field.last_pde_out = out
        field.last_pde_counters = counters
        ctx.save_for_backward(grads[0]._base)            # the one flat buffer behind the views
        ctx.specs = pack_specs(params)
        ctx.field = field
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        field = ctx.field
        if ctx.done is not None:
            torch.cuda.current_stream().wait_event(ctx.done)     # the adjoint half of the split call has filled the gradients
        if field.accumulate_grads_inplace == "arena":
            tail = field._arena_attach(field._pde_params(), [True] * fs.N_PDE, want_tail=True)
            if tail is not None and tail.numel() == ctx.saved_tensors[0].numel():
                # one launch: arena[velocity nets] += g * (gradients of the un-weighted loss); a plain read-modify-write, so the
                # backward kernels of the renders (atomic adds from other streams) are ordered behind it (_note_writer)
                field._wait_writers(True)
                tail.addcmul_(ctx.saved_tensors[0], g.to(tail.dtype).expand_as(tail))
                field._note_writer()
                field._queue_join()
                return (None,) * (_PdeFn.N_ARGS + len(ctx.specs))
        return (None,) * _PdeFn.N_ARGS + tuple(unpack_scaled(ctx.saved_tensors[0], ctx.specs, scale=g))      # one launch for all 24 tensors


class _RegFn(torch.autograd.Function):
    """`density_L1()` / `TV_loss_density(reg)` / `TV_loss_app(reg)` of the reference (tensorf_keyframe.py:188-231) on nvfi_plane_regs (regs.hip)
    instead of ~230 torch launches each.  The kernel computes all three values in one pass over the planes, and a driver calls all three per
    iteration (train_nvfi.py:203-217), so:
      forward   the first call of an iteration runs the pass and keeps the value triple; the next two find the planes unchanged (same tensors,
                same `_version`, no fused-Adam step since) and return their entry of it - one pass instead of three;
      backward  with in-place gradient accumulation (arena / caller-owned .grad) the three nodes only deposit their upstream weights; the last
                one - or the engine's end-of-backward callback, if the graph held fewer - runs ONE gradient pass with all of them
                (nvfi_plane_regs_dev: weights read from device memory, no host sync).  Under pure autograd each node has to hand its own
                gradients back to the engine, so each runs its own pass as before."""
    N_ARGS = 2      # field, which

    @staticmethod
    def forward(ctx, field, which, *planes):
        L = _lib.lib()
        rt = _rt(field)
        from .. import optim as _optim
        # nvfi_amd.optim.Adam moves the planes through raw pointers (no `_version` bump): its generation counter is part of the key, as in _frags
        key = (tuple((p.data_ptr(), p._version) for p in planes), _optim.GENERATION)
        c = rt.get("_reg_fwd")
        if c is None or c[0] != key:
            # a new pass = a new iteration: whatever an aborted backward of the previous one left behind (deposited weights, a live count that
            # never reached zero because its graph was dropped) must not leak into this one's single gradient pass
            rt.pop("_reg_pending", None)
            rt["_reg_live"] = 0
            out = torch.empty(3, device=planes[0].device)
            desc = field._desc()
            _lib.check(L.nvfi_plane_regs(C.byref(desc), 0.0, 0.0, 0.0, _lib.ptr(out), None, _stream_ptr()))
            c = (key, out, torch.cuda.current_stream())
            rt["_reg_fwd"] = c
        elif c[2] != torch.cuda.current_stream():
            torch.cuda.current_stream().wait_stream(c[2])
        ctx.field, ctx.which = field, which
        ctx.save_for_backward(*planes)
        if any(ctx.needs_input_grad):
            rt["_reg_live"] = rt.get("_reg_live", 0) + 1
        return c[1][which].clone()

    @staticmethod
    def _touched(which):
        """the planes (slots of the REG group) whose gradient term `which` reaches: L1 and TV-density the density planes, TV-app the rest"""
        return range(fs.DENSITY.stop) if which < 2 else range(fs.DENSITY.stop, fs.REG.stop)

    @staticmethod
    def _pass(field, planes, w3, grads):
        """one nvfi_plane_regs_dev gradient pass over the saved `planes` with the device-side weights w3 into `grads` (REG group)"""
        out = torch.empty(3, device=w3.device)
        G = field._grads_struct(fs.at(fs.REG, grads))
        desc = field._desc(field._params_with(fs.REG, planes))
        _lib.check(_lib.lib().nvfi_plane_regs_dev(C.byref(desc), _lib.ptr(w3), _lib.ptr(out), C.byref(G), _stream_ptr()))

    @staticmethod
    def _flush(field):
        """one gradient pass for every deposited weight (in-place modes)"""
        rt = _rt(field)
        pend = rt.pop("_reg_pending", None)
        rt["_reg_live"] = 0
        if not pend:
            return
        planes, ws = pend["planes"], pend["w"]
        touched = set()
        for which in ws:
            touched |= set(_RegFn._touched(which))
        rp = field._render_params()
        need = [k in touched for k in range(len(planes))] + [False] * (len(rp) - len(planes))
        grads, arena = field._grad_targets(rp, need)
        arena = arena and field.accumulate_grads_inplace == "arena"
        if arena:
            field._wait_writers(True)      # k_plane_regs adds with plain read-modify-writes: not next to another stream's kernels
            field._queue_join()
        else:
            grads, _ = field._grad_targets(rp, need, mode=True)
        zero = torch.zeros(1, device=planes[0].device) if len(ws) < 3 else None
        w3 = torch.cat([ws[which].reshape(1).to(torch.float32) if which in ws else zero for which in range(3)])
        _RegFn._pass(field, planes, w3, grads[fs.REG])
        if arena:
            field._note_writer()

    @staticmethod
    def backward(ctx, g):
        field, which = ctx.field, ctx.which
        planes = ctx.saved_tensors                      # the 9 regularised planes: dps[3], dpt[3], aps[3]
        rt = _rt(field)
        rt["_reg_live"] = max(rt.get("_reg_live", 1) - 1, 0)
        rt.pop("_reg_fwd", None)       # the value triple is shared by the calls of ONE iteration only (a driver that never moves the planes - bench.py's
                                        # stationary mode - must not skip next iteration's pass)
        inplace = field.accumulate_grads_inplace
        if inplace:
            # deposit; the last live node (or the end of this backward pass) runs the single gradient pass.  A field with autograd hooks on a
            # parameter gets pure autograd from _arena_attach -> the per-node path below
            hooked = inplace == "arena" and any(p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None) for p in field._arena_params())
            if not hooked:
                pend = rt.get("_reg_pending")
                if pend is None:
                    pend = rt["_reg_pending"] = dict(planes=planes, w={})
                    ref = weakref.ref(field)
                    torch.autograd.Variable._execution_engine.queue_callback(lambda: ref() is not None and _RegFn._flush(ref()))
                pend["w"][which] = g if which not in pend["w"] else pend["w"][which] + g
                if rt["_reg_live"] == 0:
                    _RegFn._flush(field)
                return (None,) * (_RegFn.N_ARGS + len(planes))
        touched = _RegFn._touched(which)
        grads = _zero_grads(planes, [k in touched for k in range(len(planes))])
        w3 = torch.zeros(3, device=g.device)
        w3[which] = g
        _RegFn._pass(field, planes, w3, grads)
        return (None,) * _RegFn.N_ARGS + tuple(grads)


class _CharFn(torch.autograd.Function):
    """nvfi_char_loss computes the value AND the unit-weight gradients of its 13 tensors (twelve planes, basis_mat) in one pass, into a private
    buffer; backward scales them by the upstream gradient (the pattern of _PdeFn)."""
    N_ARGS = 3      # field, points, t

    @staticmethod
    def forward(ctx, field, points, t, *params):
        need = ctx.needs_input_grad[_CharFn.N_ARGS:]
        grads = _zero_grads(params, need) if any(need) else [None] * len(params)
        terms, points0 = field._char_call(points, t, 1.0, grads if any(need) else None, params)
        flat = next((g._base for g in grads if g is not None), None)
        if flat is not None:
            ctx.save_for_backward(flat)
        ctx.field, ctx.need = field, list(need)
        ctx.specs = pack_specs(params)
        ctx.mark_non_differentiable(terms, points0)
        return terms[0] + terms[1], terms, points0

    @staticmethod
    def backward(ctx, g, _gt, _gp):
        if not ctx.saved_tensors:
            return (None,) * (_CharFn.N_ARGS + len(ctx.specs))
        field, saved = ctx.field, ctx.saved_tensors[0]
        if field.accumulate_grads_inplace == "arena" and all(ctx.need):
            params = field._render_params()[fs.PLANES]
            tgt = field._arena_attach(params, ctx.need)
            flat = field._arena_head(params) if tgt is not None else None
            if flat is not None:
                # one launch: arena[planes, basis_mat] += g * (unit-weight gradients); a plain read-modify-write, so it is ordered against the
                # atomic adds of the render backward on the field's side streams (_wait_writers / _note_writer), like _PdeFn's
                field._wait_writers(True)
                head = flat[:saved.numel()]
                head.addcmul_(saved, g.to(head.dtype).expand_as(head))
                field._note_writer()
                field._queue_join()
                return (None,) * (_CharFn.N_ARGS + len(ctx.specs))
        return (None,) * _CharFn.N_ARGS + tuple(unpack_scaled(saved, ctx.specs, ctx.need, g))


def _plain_grads(field, params, need, group, vel=False):
    """The plain path of a backward node: fresh zero gradients for `params` (the tensors of `group`), no arena, no side streams ->
    (grads, nvfi_grads struct over them)"""
    grads = _zero_grads(params, need)
    if vel:
        return grads, field._grads_struct_vel(fs.at(group, grads, fs.N_PDE))
    return grads, field._grads_struct(fs.at(group, grads))


class _AdvectFn(torch.autograd.Function):
    """autograd boundary around nvfi_integrate_pos / nvfi_advect_grad (include/nvfi_hip.h) for host-scalar times.  The forward IS
    field.integrate_pos and saves only the positions: the backward runs the warp again in training form, chunk by chunk on one workspace of at
    most `max_ws` bytes (the stash is ~10.8 KB per point and RK2 step), and accumulates the net's gradients over the chunks."""
    N_ARGS = 5      # field, x, t, t_target, max_ws

    @staticmethod
    def forward(ctx, field, x, t, t_target, max_ws, *params):
        tt = torch.full((x.shape[0],), t, dtype=torch.float32, device=x.device)
        bb = torch.full((x.shape[0],), t_target, dtype=torch.float32, device=x.device)
        xk = field.integrate_pos(x, tt, bb)
        ctx.field, ctx.t, ctx.t_target, ctx.max_ws = field, t, t_target, int(max_ws)
        ctx.save_for_backward(x, *params)
        ctx.set_materialize_grads(False)
        return xk

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, *params = ctx.saved_tensors
        if g is None:
            return (None,) * (_AdvectFn.N_ARGS + len(params))
        L = _lib.lib()
        field = ctx.field
        desc = field._desc(field._params_with(fs.WEIGHT_NET, params))
        grads, G = _plain_grads(field, params, ctx.needs_input_grad[_AdvectFn.N_ARGS:], fs.PDE_WEIGHT_NET, vel=True)
        g = g.reshape(-1, 3).contiguous().float()
        N = x.shape[0]
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        t, t1 = ctx.t, ctx.t_target

        def nbytes(n):
            return _lib.bytes_of(L.nvfi_advect_grad_workspace_bytes, C.byref(desc), n, t, t1)

        chunk, ws_bytes, chunks = _lib.plan_chunks(nbytes, N, ctx.max_ws, "advect", unit="point")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        field.last_advect_chunks = chunks
        field.last_advect_workspace_bytes = ws.numel()
        for i in range(0, chunks * chunk, max(chunk, 1)):
            n = min(chunk, N - i)
            _lib.check(L.nvfi_advect_grad(C.byref(desc), n, _lib.ptr(x[i:i + n]), t, t1, _lib.ptr(g[i:i + n]),
                                          None if gx is None else _lib.ptr(gx[i:i + n]), C.byref(G), _lib.ptr(ws), ws.numel(), _stream_ptr()))
        return (None, gx, None, None, None) + tuple(grads)


class _AdvectPtFn(torch.autograd.Function):
    """autograd boundary around nvfi_integrate_pos / nvfi_advect_grad_pt (include/nvfi_hip_advect_pt.h) for per-point times, built like _AdvectFn.  The
    forward IS field.integrate_pos; it also runs nvfi_advect_pt_steps and reads the 66-bin histogram of the step counts - THE ONE HOST
    SYNCHRONISATION of the call (a point beyond 64 steps is refused here, before anything else, and the backward plans from the histogram
    alone).  The backward's cost follows the sum of the steps, not N x the largest: the points are sorted by step count (descending, stable),
    every step count is planned on its own with `_lib.plan_chunks` under `max_ws` bytes and launched with that count as its max_steps, and
    the zero-step tail launches nothing (g_x = g there).  The times get no gradient."""
    N_ARGS = 5      # field, x, t, t_target, max_ws

    @staticmethod
    def forward(ctx, field, x, t, t_target, max_ws, *params):
        L = _lib.lib()
        N = x.shape[0]
        desc = field._desc()
        steps = torch.empty(N, dtype=torch.int32, device=x.device)
        hist = torch.empty(66, dtype=torch.int64, device=x.device)
        _lib.check(L.nvfi_advect_pt_steps(C.byref(desc), N, _lib.ptr(t), _lib.ptr(t_target), _lib.ptr(steps), _lib.ptr(hist), _stream_ptr()))
        hist = hist.tolist()                     # the host read
        if hist[65]:
            raise _lib.NvfiError(f"libnvfi_hip error 2: advect_pt: {hist[65]} point(s) need more than 64 RK2 steps (refused, not truncated)")
        xk = field.integrate_pos(x, t, t_target)
        ctx.field, ctx.max_ws, ctx.hist = field, int(max_ws), hist[:65]
        ctx.save_for_backward(x, t, t_target, steps, *params)
        ctx.set_materialize_grads(False)
        return xk

    @staticmethod
    def plan(nbytes, hist, max_ws):
        """[(first, n, max_steps)] over the points sorted by step count, descending, and the bytes of the largest chunk: one plan_chunks per
        step count that occurs; the zero-step points come last as one entry that launches nothing"""
        chunks, first, ws_bytes = [], 0, 0
        for s in range(len(hist) - 1, 0, -1):
            if not hist[s]:
                continue
            chunk, nb, _ = _lib.plan_chunks(lambda n: nbytes(n, s), hist[s], max_ws, "advect_pt", unit="point")
            ws_bytes = max(ws_bytes, nb)
            for i in range(0, hist[s], chunk):
                chunks.append((first + i, min(chunk, hist[s] - i), s))
            first += hist[s]
        if hist[0]:
            chunks.append((first, hist[0], 0))
        return chunks, ws_bytes

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, t, t1, steps, *params = ctx.saved_tensors
        if g is None:
            return (None,) * (_AdvectPtFn.N_ARGS + len(params))
        L = _lib.lib()
        field = ctx.field
        desc = field._desc(field._params_with(fs.WEIGHT_NET, params))
        grads, G = _plain_grads(field, params, ctx.needs_input_grad[_AdvectPtFn.N_ARGS:], fs.PDE_WEIGHT_NET, vel=True)
        g = g.reshape(-1, 3).contiguous().float()
        want_gx = ctx.needs_input_grad[1]
        chunks, ws_bytes = _AdvectPtFn.plan(lambda n, s: _lib.bytes_of(L.nvfi_advect_grad_pt_workspace_bytes, C.byref(desc), n, s), ctx.hist, ctx.max_ws)
        field.last_advect_pt_chunks = [(n, s) for _, n, s in chunks]
        field.last_advect_pt_workspace_bytes = ws_bytes
        if not any(s for _, _, s in chunks):      # nobody moves: the gradient passes through, the net gets exact zeros
            return (None, g.clone() if want_gx else None, None, None, None) + tuple(grads)
        order = torch.argsort(steps, descending=True, stable=True)
        xs, ts, t1s, gs = x[order], t[order], t1[order], g[order]
        gxs = gs.clone() if want_gx else None     # the zero-step tail keeps g
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        for i, n, s in chunks:
            if s == 0:
                continue
            _lib.check(L.nvfi_advect_grad_pt(C.byref(desc), n, _lib.ptr(xs[i:i + n]), _lib.ptr(ts[i:i + n]), _lib.ptr(t1s[i:i + n]), s,
                                             _lib.ptr(gs[i:i + n]), None if gxs is None else _lib.ptr(gxs[i:i + n]), C.byref(G), None,
                                             _lib.ptr(ws), ws.numel(), _stream_ptr()))
        gx = None
        if want_gx:
            gx = torch.empty_like(gxs)
            gx[order] = gxs
        return (None, gx, None, None, None) + tuple(grads)


class _ShadeFn(torch.autograd.Function):
    """autograd boundary around nvfi_render_mlp / nvfi_render_mlp_grad (include/nvfi_hip.h), built like _AdvectFn.  The forward IS
    field._render_module_call and saves only the three inputs and the six tensors of renderModule.mlp (none under SH shading): the backward
    runs the forward again in stash form, chunk by chunk on one workspace of at most `max_ws` bytes (~3 KB per point + 51 MB of slabs), and
    accumulates the MLP's gradients over the chunks into buffers cleared here."""
    N_ARGS = 5      # field, pts, viewdirs, features, max_ws

    @staticmethod
    def forward(ctx, field, pts, viewdirs, features, max_ws, *params):
        rgb = field._render_module_call(pts, viewdirs, features)
        ctx.field, ctx.max_ws = field, int(max_ws)
        ctx.save_for_backward(pts, viewdirs, features, *params)
        ctx.set_materialize_grads(False)
        return rgb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..utils import field_lookup as fl
        x, v, fe, *params = ctx.saved_tensors
        if g is None:
            return (None,) * (_ShadeFn.N_ARGS + len(params))
        field = ctx.field
        need = ctx.needs_input_grad[_ShadeFn.N_ARGS:]
        grads, G = [], None
        desc = field._desc(field._params_with(fs.RENDER_MLP, params) if params else None)
        if params and any(need):
            grads, G = _plain_grads(field, params, need, fs.RENDER_MLP)
        elif params:
            grads = [None] * len(params)
        g = g.reshape(-1, 3).contiguous().float()
        N = x.shape[0]
        want_x, want_v, want_f = ctx.needs_input_grad[1:4]
        gx = torch.empty_like(x) if want_x else None
        gv = torch.empty_like(v) if want_v else None
        gf = torch.empty_like(fe) if want_f else None
        chunk, ws_bytes, chunks = _lib.plan_chunks(lambda n: fl.render_mlp_grad_workspace_bytes(desc, n), N, ctx.max_ws, "shade", unit="point")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        field.last_shade_chunks = chunks
        field.last_shade_workspace_bytes = ws.numel()
        for i in range(0, chunks * chunk, max(chunk, 1)):
            s = slice(i, min(i + chunk, N))
            fl.render_mlp_grad_raw(desc, x[s], v[s], fe[s], g[s], g_features=None if gf is None else gf[s], g_xyz=None if gx is None else gx[s],
                                   g_view=None if gv is None else gv[s], grads=G, workspace=ws)
        return (None, gx, gv, gf, None) + tuple(grads)


class _DensityLookupFn(torch.autograd.Function):
    """autograd boundary around nvfi_density_at / nvfi_density_grad (include/nvfi_hip.h).  The forward IS field.compute_densityfeature and saves
    only the points and the six density planes: the backward reads the taps again (no stash) and computes only what autograd asks for."""
    N_ARGS = 2      # field, q

    @staticmethod
    def forward(ctx, field, q, *planes):
        feat = field.compute_densityfeature(q)
        ctx.field = field
        ctx.save_for_backward(q, *planes)
        ctx.set_materialize_grads(False)
        return feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..utils import field_lookup as fl
        return _lookup_backward(ctx, g, _DensityLookupFn.N_ARGS, fs.DENSITY, fl.density_grad_raw)


class _AppLookupFn(torch.autograd.Function):
    """autograd boundary around nvfi_appfeat_at / nvfi_appfeat_grad (include/nvfi_hip.h): compute_appfeature with gradients to the points, the
    six appearance planes and basis_mat.weight; built like _DensityLookupFn."""
    N_ARGS = 2      # field, q

    @staticmethod
    def forward(ctx, field, q, *params):
        from ..utils import field_lookup as fl
        feat = fl.appfeat_raw(field._desc(), q)
        ctx.field = field
        ctx.save_for_backward(q, *params)
        ctx.set_materialize_grads(False)
        return feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..utils import field_lookup as fl
        return _lookup_backward(ctx, g, _AppLookupFn.N_ARGS, fs.APP, fl.appfeat_grad_raw)


def _lookup_backward(ctx, g, n_args, group, raw):
    """the shared backward of the two point lookups: the saved tensors of `group` stand in the descriptor, `raw` (utils.field_lookup) does the call"""
    q, *params = ctx.saved_tensors
    if g is None:
        return (None,) * (n_args + len(params))
    field = ctx.field
    desc = field._desc(field._params_with(group, params))
    need = ctx.needs_input_grad[n_args:]
    grads, G = _plain_grads(field, params, need, group)
    gq = raw(desc, q, g, g_xyzt=True if ctx.needs_input_grad[1] else None, grads=G if any(need) else None)
    return (None, gq) + tuple(grads)


class _FlowLossFn(torch.autograd.Function):
    """autograd boundary around nvfi_flow_loss_fwd / nvfi_flow_loss_bwd (include/nvfi_hip.h), built like _AdvectFn: the forward runs behind the
    training render whose backward node `node` still holds its workspace and forms the value, d loss / d weights and the per-entry gradient at
    the displaced points in the call's own workspace; the backward runs the adjoint of integrate_pos chunk by chunk on that workspace and hands
    d loss / d weights to autograd, which carries it into _RenderFn.backward as g_weights."""
    N_ARGS = 10     # field, weights, node, dt, camera, target, valid, kind, huber_delta, max_ws

    @staticmethod
    def forward(ctx, field, weights, node, dt, camera, target, valid, kind, huber_delta, max_ws, *params):
        from ..utils import flow_loss as fl
        rays_o, rays_d, w_saved = node.saved_tensors[:3]
        desc = field._desc(field._params_with(fs.WEIGHT_NET, params))
        desc.vel_fp16 = node.vel_fp16
        want_gw = ctx.needs_input_grad[1]
        call = fl.flow_loss_raw(desc, node.ws, node.flags, rays_o, rays_d, w_saved, node.t, dt, camera, target, valid=valid, kind=kind,
                                huber_delta=huber_delta, g_weights=None if want_gw else False, max_workspace_bytes=max_ws)
        field.last_flow_chunks, field.last_flow_workspace_bytes = call["chunks"], call["workspace"].numel()
        field.last_flow2d, field.last_flow_n = call["flow2d"], call["loss"][1]
        ctx.field, ctx.call, ctx.vel_fp16 = field, call, node.vel_fp16
        ctx.save_for_backward(*params)
        return call["loss"][0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..utils import flow_loss as fl
        params = list(ctx.saved_tensors)
        field, call = ctx.field, ctx.call
        if call is None:
            raise ValueError("flow_loss: the workspace of this call was released by its first backward; a second backward needs a new flow_loss call")
        desc = field._desc(field._params_with(fs.WEIGHT_NET, params))
        desc.vel_fp16 = ctx.vel_fp16
        need = ctx.needs_input_grad[_FlowLossFn.N_ARGS:]
        grads, G = _plain_grads(field, params, need, fs.PDE_WEIGHT_NET, vel=True)
        if any(need):
            fl.flow_loss_backward_raw(desc, call, G)
        g = g.detach().float()
        for gr in grads:                           # the upstream gradient never visits the host
            if gr is not None:
                gr.mul_(g)
        g_w = call["g_weights"] * g if ctx.needs_input_grad[1] else None
        ctx.call = None
        return (None, g_w) + (None,) * (_FlowLossFn.N_ARGS - 2) + tuple(grads)


class _MaskLossFn(torch.autograd.Function):
    """autograd boundary around nvfi_mask_loss_fwd / nvfi_mask_loss_bwd (include/nvfi_hip.h), built like _FlowLossFn: the forward runs behind
    the training render whose backward node `node` still holds its workspace and forms the value, the mask map, d loss / d weights and the
    per-ray g_q in the call's own workspace; the backward runs the MaskField adjoint chunk by chunk on that workspace and hands
    d loss / d weights to autograd, which carries it into _RenderFn.backward as g_weights.  params: the ten MaskField tensors."""
    N_ARGS = 8      # field, weights, node, mask_field, target, kind, eps, max_ws

    @staticmethod
    def forward(ctx, field, weights, node, mask_field, target, kind, eps, max_ws, *params):
        from ..utils import mask_loss as ml
        from .mask_field import _mask_desc
        w_saved = node.saved_tensors[2]
        desc = field._desc()
        desc.vel_fp16 = node.vel_fp16
        params_c = [p.detach().contiguous() for p in params]
        md = _mask_desc(mask_field, params_c)
        want_gw = ctx.needs_input_grad[1]
        call = ml.mask_loss_raw(desc, md, node.ws, node.flags, w_saved, node.t, target, kind=kind, eps=eps,
                                g_weights=None if want_gw else False, max_workspace_bytes=max_ws)
        field.last_mask_chunks, field.last_mask_workspace_bytes = call["chunks"], call["workspace"].numel()
        field.last_mask_map, field.last_mask_n = call["mask_map"], call["loss"][1]
        ctx.mask_field, ctx.call, ctx.params_c = mask_field, call, params_c
        return call["loss"][0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..utils import mask_loss as ml
        from .mask_field import _mask_desc
        call = ctx.call
        if call is None:
            raise ValueError("mask_loss: the workspace of this call was released by its first backward; a second backward needs a new mask_loss call")
        need = ctx.needs_input_grad[_MaskLossFn.N_ARGS:]
        grads = [torch.zeros_like(p) if n else None for p, n in zip(ctx.params_c, need)]
        if any(need):
            ml.mask_loss_backward_raw(_mask_desc(ctx.mask_field, ctx.params_c), call, ml.mask_grads_struct(grads))
        g = g.detach().float()
        for gr in grads:                           # the upstream gradient never visits the host
            if gr is not None:
                gr.mul_(g)
        g_w = call["g_weights"] * g if ctx.needs_input_grad[1] else None
        ctx.call = None
        return (None, g_w) + (None,) * (_MaskLossFn.N_ARGS - 2) + tuple(grads)
