"""Where a backward of the field writes: the flat gradient format, the gradient arena, the choice of the write target and the side streams
that order the writers (the host side of plain-autograd drivers; TensorVMKeyframeTimeKplane mixes FieldGrads in)."""
import weakref

import torch

from . import field_slots as fs

# per-field runtime state that must not travel with copy.deepcopy / pickle of the module (HIP streams, events, pinned buffers, the
# gradient arena): kept beside the module, keyed weakly
_RUNTIME = weakref.WeakKeyDictionary()


def _rt(field):
    d = _RUNTIME.get(field)
    if d is None:
        d = _RUNTIME[field] = {}
    return d


# ---------------------------------------------------------------------- the flat gradient format
def round64(n):
    """n rounded up to 64 elements: 256-byte aligned pieces of one fp32 buffer"""
    return (n + 63) // 64 * 64


def pack_specs(params):
    """what the flat format keeps of a parameter: (shape, strides); None stays None"""
    return [None if p is None else (p.shape, p.stride()) for p in params]


def pack_layout(specs, need=None):
    """(offsets, total) in elements of the flat gradient buffer of `specs`: the tensors `need` names, in order, each starting on a multiple of
    64 elements (the plane-gradient kernels use 16-byte accesses)"""
    need = [True] * len(specs) if need is None else list(need)
    offs, total = [], 0
    for s, n in zip(specs, need):
        offs.append(total)
        if n:
            total += round64(s[0].numel())
    return offs, total


def pack_views(flat, specs, need=None, offs=None):
    """Views of the flat buffer `flat`, None where `need` is false: each with its parameter's shape and strides (the planes are stored
    channel-last under an NCHW shape; all parameters are dense).  offs: the offsets of pack_layout(specs, need), when the caller has them"""
    need = [True] * len(specs) if need is None else list(need)
    offs = pack_layout(specs, need)[0] if offs is None else offs
    return [flat[o:o + s[0].numel()].as_strided(s[0], s[1]) if n else None for s, n, o in zip(specs, need, offs)]


def _zero_grads(params, need=None):
    """Fresh zero gradients for `params` (None where `need` is false) as views of ONE zero-filled buffer: one fill launch per backward
    node instead of one per parameter (the plain-autograd path of the reference's training loop is bound by the host's launch rate)."""
    need = [True] * len(params) if need is None else list(need)
    specs = pack_specs(params)
    offs, total = pack_layout(specs, need)
    if total == 0:
        return [None] * len(params)
    ref = next(p for p, n in zip(params, need) if n)
    return pack_views(torch.zeros(total, dtype=ref.dtype, device=ref.device), specs, need, offs)


def unpack_scaled(flat, specs, need=None, scale=None):
    """The gradients a flat buffer holds, times `scale`: one launch for all of them"""
    return pack_views(flat if scale is None else flat * scale, specs, need)


class FieldGrads:
    """gradient arena + write target + side streams of the field"""

    def _arena_params(self):
        ps = self._render_params()
        if self.use_vel:
            ps = ps + self._pde_params()[fs.PDE_A_WEIGHT_NET]    # + the acceleration net: the PDE parameters are then the last N_PDE entries
        return [p for p in ps if p is not None]

    def _arena_attach(self, params, need, want_tail=False):
        """Gradient targets for `params` (None where `need` is false) as views of the field's persistent flat buffer.  A parameter whose
        .grad is None gets its (zeroed) view attached; when that is true for every parameter of the field - the state a driver's
        `zero_grad(set_to_none=True)` leaves behind - the whole buffer is cleared with ONE fill.  A .grad the caller put there is used
        as it is when its layout matches the parameter's; otherwise None is returned and the call falls back to pure autograd.
        want_tail: return the flat view that covers the 24 velocity-net tensors instead (they are contiguous at the end)."""
        ps = self._arena_params()
        # a hook on any parameter (tensor hooks, post-accumulate-grad hooks: DDP, optimiser-in-backward, clipping) only fires when the
        # engine itself accumulates the gradient: such a field gets pure autograd
        for p in ps:
            if p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
                return None
        key = tuple((id(p), tuple(p.shape), p.stride()) for p in ps)
        a = _rt(self).get("_arena")
        if a is None or a["key"] != key or a["flat"].device != ps[0].device:
            specs = pack_specs(ps)
            offs, total = pack_layout(specs)
            flat = torch.zeros(total, dtype=torch.float32, device=ps[0].device)
            views = {id(p): v for p, v in zip(ps, pack_views(flat, specs, offs=offs))}
            a = dict(key=key, flat=flat, views=views, offs=offs, params=ps, event=None,
                     tail=flat[offs[-fs.N_PDE]:] if (self.use_vel and len(ps) >= fs.N_PDE) else None)
            _rt(self)["_arena"] = a
        # only the parameters THIS node differentiates are attached: a parameter no term of the loss reaches keeps .grad = None and the
        # optimiser skips it, exactly as under pure autograd
        wanted = {id(p) for p, n in zip(params, need) if n and p is not None}
        idx = [i for i, p in enumerate(a["params"]) if id(p) in wanted and p.requires_grad and p.grad is None]
        if a["event"] is not None:
            torch.cuda.current_stream().wait_event(a["event"])      # fills queued by nodes that ran on other streams
        if idx:
            lo, hi = idx[0], idx[-1]
            with torch.no_grad():
                if len(idx) == hi - lo + 1:        # a contiguous run of the buffer (the usual case): ONE fill
                    end = a["offs"][hi + 1] if hi + 1 < len(a["offs"]) else a["flat"].numel()
                    a["flat"][a["offs"][lo]:end].zero_()
                else:
                    for i in idx:
                        a["views"][id(a["params"][i])].zero_()
            for i in idx:
                p = a["params"][i]
                p.grad = a["views"][id(p)]
            ev = torch.cuda.Event()
            ev.record()
            a["event"] = ev            # other streams' backward nodes order themselves behind the fill
        out = []
        for p, n in zip(params, need):
            if not n or p is None:
                out.append(None)
                continue
            g = p.grad
            if g is None or g.stride() != p.stride() or g.dtype != torch.float32 or g.device != p.device:
                return None
            out.append(g)
        if want_tail:
            vs = self._pde_params()
            ok = a["tail"] is not None and all(p.grad is a["views"].get(id(p)) for p in vs)
            return a["tail"] if ok else None
        return out

    def _arena_head(self, params):
        """The arena's flat buffer when `params` ARE its first tensors and every one of them has its arena view attached as .grad (after
        an _arena_attach of them): their gradients are then the head of the buffer, in the flat format - or None"""
        a = _rt(self).get("_arena")
        if a is None or not all(x is y for x, y in zip(a["params"][:len(params)], params)) or not all(p.grad is a["views"].get(id(p)) for p in params):
            return None
        return a["flat"]

    def _grad_targets(self, params, need, mode=None):
        """(grads, inplace): where a backward node writes the gradients of `params` (None where `need` is false) under `mode`, by default
        the field's accumulate_grads_inplace:
          "arena"   views of the field's flat buffer (_arena_attach, with its wait for the fills of other streams); a field with an
                    autograd hook on a parameter, or a foreign .grad of another layout, gets (None, False)
          True      the caller-owned .grad of each parameter, created with zeros_like where it is missing
          False     (None, False): the caller takes fresh zeros (_zero_grads) and hands them to the engine
        Ordering the writers (_wait_writers / _note_writer / _queue_join) stays with the caller."""
        mode = self.accumulate_grads_inplace if mode is None else mode
        if mode == "arena":
            grads = self._arena_attach(params, need)
            return grads, grads is not None
        if not mode:
            return None, False
        # kernels accumulate (+=) straight into the parameters' .grad (e.g. views of one flat GradBucket buffer):
        # no zero-fill, no AccumulateGrad add per tensor.  Autograd then sees "no gradient" for these inputs.
        grads = []
        for p, n in zip(params, need):
            if not n:
                grads.append(None)
                continue
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad)
        return grads, True

    def _side_stream(self, kind):
        pool = _rt(self).get("_side_pool")
        if pool is None:
            dev = self.aabb.device
            pool = dict(r=[torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)], p=torch.cuda.Stream(device=dev), k=0)
            _rt(self)["_side_pool"] = pool
        if kind == "p":
            return pool["p"]
        pool["k"] += 1
        return pool["r"][pool["k"] & 1]

    def _use_side_streams(self):
        return (self.auto_overlap and self.accumulate_grads_inplace == "arena" and self.aabb.is_cuda and torch.is_grad_enabled()
                and not torch.cuda.is_current_stream_capturing())

    def _note_writer(self):
        """The current stream just queued a non-atomic read-modify-write of gradient memory: later backward nodes (any stream) wait for it."""
        ev = torch.cuda.Event()
        ev.record()
        _rt(self).setdefault("_writers", []).append(ev)

    def _wait_writers(self, also_side_streams=False):
        cur = torch.cuda.current_stream()
        for ev in _rt(self).get("_writers", ()):
            cur.wait_event(ev)
        if also_side_streams:          # a non-atomic writer must not run next to ANY other backward kernel of the field
            pool = _rt(self).get("_side_pool")
            if pool is not None:
                for st in pool["r"] + [pool["p"]]:
                    if st != cur:
                        cur.wait_stream(st)

    def _queue_join(self):
        """Once per backward pass: when the engine has run every node, the stream of the thread that called backward() waits for the
        field's side streams - the optimiser step that follows then sees complete gradients (the engine itself only orders the
        gradients it is handed, and in-place accumulation hands it none)."""
        if _rt(self).get("_join_pending"):
            return
        _rt(self)["_join_pending"] = True
        ref = weakref.ref(self)

        def join():
            f = ref()
            if f is None:
                return
            _rt(f)["_join_pending"] = False
            _rt(f)["_writers"] = []
            pool = _rt(f).get("_side_pool")
            if pool is not None:
                cur = torch.cuda.current_stream()
                for st in pool["r"] + [pool["p"]]:
                    cur.wait_stream(st)

        from torch.autograd import Variable
        Variable._execution_engine.queue_callback(join)
