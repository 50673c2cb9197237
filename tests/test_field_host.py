"""The host-side definitions every caller of the library shares, as far as they can be checked without a device: the slot table of the
field's tensors (models/field_slots.py) against the struct layout of include/nvfi_hip.h as _lib mirrors it, the flat gradient format
(models/field_grads.py) and the chunk planner of the stash-bound adjoints (_lib.plan_chunks, utils.flow_loss.flow_loss_plan)."""
import ctypes as C

import pytest
import torch

# struct member -> slots of the list, written out from nvfi_field_desc / nvfi_grads (include/nvfi_hip.h) and _render_params / _pde_params
RENDER = {"dps": [0, 1, 2], "dpt": [3, 4, 5], "aps": [6, 7, 8], "apt": [9, 10, 11], "basis": 12, "rW": [13, 15, 17], "rb": [14, 16, 18],
          "vW": [19, 21, 23, 25, 27, 29], "vb": [20, 22, 24, 26, 28, 30]}
PDE = {"vW": [0, 2, 4, 6, 8, 10], "vb": [1, 3, 5, 7, 9, 11], "aW": [12, 14, 16, 18, 20, 22], "ab": [13, 15, 17, 19, 21, 23]}


def _slots(members):
    return [k for _, s in members for k in ([s] if isinstance(s, int) else s)]


def test_slot_groups_tile_the_lists_in_struct_order():
    from nvfi_amd import _lib
    from nvfi_amd.models import field_slots as fs
    fields = [n for n, _ in _lib.Grads._fields_]
    assert [n for n, _ in fs.RENDER_MEMBERS] == fields[:9] and [n for n, _ in fs.PDE_MEMBERS] == fields[7:]
    assert sorted(_slots(fs.RENDER_MEMBERS)) == list(range(fs.N_RENDER)) == list(range(31))
    assert sorted(_slots(fs.PDE_MEMBERS)) == list(range(fs.N_PDE)) == list(range(24))
    assert fs.PDE_A_MEMBERS == fs.PDE_MEMBERS[2:]
    r31, r24 = list(range(31)), list(range(24))
    assert r31[fs.DENSITY] + r31[fs.APP] + r31[fs.RENDER_MLP] + r31[fs.WEIGHT_NET] == r31
    assert r31[fs.PLANES] == r31[fs.DENSITY] + r31[fs.APP] == r31[fs.FACTOR_PLANES] + [12]
    assert r31[fs.REG] == list(range(9)) and r31[fs.LINEARS] == [12] + r31[fs.RENDER_MLP] + r31[fs.WEIGHT_NET]
    assert r24[fs.PDE_WEIGHT_NET] + r24[fs.PDE_A_WEIGHT_NET] == r24 and len(r24[fs.PDE_WEIGHT_NET]) == len(r31[fs.WEIGHT_NET]) == 12
    assert fs.at(fs.APP, list("abcdefg")) == [None] * 6 + list("abcdefg") + [None] * 18
    assert fs.at(fs.PDE_WEIGHT_NET, r24[:12], fs.N_PDE) == r24[:12] + [None] * 12
    with pytest.raises(ValueError):
        fs.at(fs.DENSITY, [1, 2, 3])


def _members_of(st):
    return {n: (getattr(st, n) if isinstance(getattr(st, n), (int, type(None))) else list(getattr(st, n)))
            for n in ("dps", "dpt", "aps", "apt", "basis", "rW", "rb", "vW", "vb", "aW", "ab")}


@pytest.mark.parametrize("struct", ["Grads", "FieldDesc"])
def test_fill_puts_every_slot_into_the_member_the_header_names(struct):
    from nvfi_amd import _lib
    from nvfi_amd.models import field_slots as fs
    make = getattr(_lib, struct)

    def fake(k):
        return C.c_void_p(1000 + k)

    def want(table, n):
        out = {m: None if m == "basis" else [None] * len(getattr(make(), m)) for m in _members_of(make())}
        for m, s in table.items():
            out[m] = (1000 + s if s < n else None) if isinstance(s, int) else [1000 + k if k < n else None for k in s]
        return out

    assert _members_of(fs.fill(make(), [fake(k) for k in range(31)], ptr=lambda x: x)) == want(RENDER, 31)
    assert _members_of(fs.fill(make(), [fake(k) for k in range(24)], fs.PDE_MEMBERS, ptr=lambda x: x)) == want(PDE, 24)
    assert _members_of(fs.fill(make(), [fake(k) for k in range(24)], fs.PDE_A_MEMBERS, ptr=lambda x: x)) == want({m: PDE[m] for m in ("aW", "ab")}, 24)
    # a list that ends early (a field without velocity net: 19 tensors; the 13 plane tensors) leaves NULL behind it, None stays NULL
    for n in (19, 13, 9):
        assert _members_of(fs.fill(make(), [fake(k) for k in range(n)], ptr=lambda x: x)) == want(RENDER, n)
    holes = [None if k in (1, 12, 14) else fake(k) for k in range(31)]
    got = _members_of(fs.fill(make(), holes, ptr=lambda x: x))
    assert got["dps"] == [1000, None, 1002] and got["basis"] is None and got["rb"] == [None, 1016, 1018] and got["vb"] == want(RENDER, 31)["vb"]


def _params():
    return [torch.zeros(1, 5, 3, 7).contiguous(memory_format=torch.channels_last), torch.zeros(8, 8), torch.zeros(65), torch.zeros(1)]


@pytest.mark.parametrize("need", [(True, True, True, True), (True, False, True, True), (False, False, False, False)])
def test_flat_gradient_format(need):
    from nvfi_amd.models import field_grads as fg
    params = _params()
    views = fg._zero_grads(params, need)
    if not any(need):
        assert views == [None] * 4
        return
    kept = [(p, v) for p, v, n in zip(params, views, need) if n]
    assert all(v is None for v, n in zip(views, need) if not n)
    base = kept[0][1]._base
    assert base.dim() == 1 and not base.any() and base.numel() == sum(fg.round64(p.numel()) for p, _ in kept)
    at = 0
    for p, v in kept:
        assert v._base is base and v.storage_offset() == at and at % 64 == 0
        assert v.shape == p.shape and v.stride() == p.stride() and v.dtype == p.dtype
        at += fg.round64(p.numel())
    assert fg._zero_grads(params)[1].storage_offset() == 128 and fg.round64(0) == 0 and fg.round64(64) == 64 and fg.round64(65) == 128
    # the same format read back: views of a given flat buffer, scaled by the upstream gradient
    specs = fg.pack_specs(params)
    offs, total = fg.pack_layout(specs, need)
    assert total == base.numel() and [o for o, n in zip(offs, need) if n] == [v.storage_offset() for _, v in kept]
    flat = torch.arange(total, dtype=torch.float32) + 1
    g = torch.tensor(0.3)
    plain, scaled = fg.pack_views(flat, specs, need), fg.unpack_scaled(flat, specs, need, g)
    for p, v, s, n in zip(params, plain, scaled, need):
        assert (v is None and s is None) if not n else (v._base is flat and s.shape == p.shape and s.stride() == p.stride() and torch.equal(s, v * g))


def _sizes(b0, k, jump_at=None, jump=0):
    calls = []

    def nbytes(n):
        calls.append(n)
        return b0 + k * -(-n // 128) + (jump if jump_at is not None and n > jump_at else 0)
    return nbytes, calls


@pytest.mark.parametrize("jump_at,jump", [(None, 0), (1024, 5000), (300, 12345)])
@pytest.mark.parametrize("cap", [0, 1, 127, 128, 129, 1000, 4096, 100001])
def test_plan_chunks_properties(cap, jump_at, jump):
    from nvfi_amd import _lib
    b0, k = 4096, 1000
    nbytes, calls = _sizes(b0, k, jump_at, jump)
    one = nbytes(128)
    for mx in (one, one + 1, one + k - 1, one + 3 * k, one + 7 * k + jump, nbytes(1024) + jump, nbytes(cap), nbytes(cap) - 1, 1 << 40):
        if mx < one:
            continue
        chunk, nb, chunks = _lib.plan_chunks(nbytes, cap, mx, "advect", unit="point")
        assert nb == nbytes(chunk) and chunks == (-(-cap // chunk) if cap else 0)
        if nbytes(cap) <= mx:
            assert chunk == cap and chunks == (1 if cap else 0)
        else:
            assert chunk % 128 == 0 and 128 <= chunk < cap and nbytes(chunk) <= mx < nbytes(chunk + 128), (cap, mx, chunk)
    if cap > 128:
        for what, unit, msg in (("advect", "point", "advect: max_workspace_bytes=%d is below the %d bytes one 128-point group needs"),
                                ("flow loss", "entry", "flow loss: max_workspace_bytes=%d is below the %d bytes one 128-entry group needs")):
            with pytest.raises(_lib.NvfiError) as e:
                _lib.plan_chunks(nbytes, cap, one - 1, what, unit=unit)
            assert str(e.value) == msg % (one - 1, one)


def test_plan_chunks_steps_down_from_an_overshooting_guess():
    from nvfi_amd import _lib
    nbytes, calls = _sizes(4096, 1000, 1024, 5000)
    mx = nbytes(1024) + 4000          # the affine guess (no jump in the 128 and 256 plans) lands at 1536, which the jump makes too large
    del calls[:]
    assert _lib.plan_chunks(nbytes, 100000, mx, "advect")[0] == 1024
    assert calls[:3] == [100000, 128, 256] and calls[3:-1] == [1536, 1408, 1280, 1152, 1024] and calls[-1] == 1024


def test_flow_loss_plan_on_the_pinned_descriptor():
    """the library's own size call (host only) behind flow_loss_plan, with a limit that forces at least three chunks"""
    from nvfi_amd import _lib
    from nvfi_amd.utils.flow_loss import flow_loss_plan
    from test_flowloss_abi import TS, _desc
    d, R, t, dt = _desc(), 2048, 0.3, TS / 4
    cap = R * d.n_samples

    def nbytes(n):
        return _lib.bytes_of(_lib.lib().nvfi_flow_loss_workspace_bytes, C.byref(d), C.c_int64(R), C.c_float(t), C.c_float(dt), C.c_int64(n))

    assert flow_loss_plan(d, R, t, dt, 1 << 40) == (cap, nbytes(cap), 1)
    mx = nbytes(cap // 3)
    chunk, nb, chunks = flow_loss_plan(d, R, t, dt, mx)
    print(f"flow_loss_plan: cap {cap}, limit {mx} -> chunk {chunk}, {nb} bytes, {chunks} chunks")
    assert chunks >= 3 and chunks == -(-cap // chunk) and nb == nbytes(chunk)
    assert chunk % 128 == 0 and nbytes(chunk) <= mx < nbytes(chunk + 128)
    with pytest.raises(_lib.NvfiError, match="flow loss: max_workspace_bytes=1000 is below the"):
        flow_loss_plan(d, R, t, dt, 1000)
