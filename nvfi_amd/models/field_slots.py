"""The slot order of the field's tensors, written down once (include/nvfi_hip.h: nvfi_field_desc / nvfi_grads).

The render path sees 31 tensors in nvfi_field_desc order (TensorVMKeyframeTimeKplane._render_params), the PDE term 24 (_pde_params:
weight_net, then a_weight_net).  Everything that slices such a list, pads it or turns it into the pointer members of a ctypes struct goes
through the names below: a wrong copy of one of these numbers does not raise, it writes a gradient into the wrong tensor."""
from .. import _lib

# ---- the 31 render tensors: named groups (slices of the list)
N_RENDER = 31
DENSITY = slice(0, 6)            # density_plane_space[3], density_plane_time[3]
REG = slice(0, 9)                # + app_plane_space[3]: what nvfi_plane_regs regularises
APP = slice(6, 13)               # app_plane_space[3], app_plane_time[3], basis_mat.weight
FACTOR_PLANES = slice(0, 12)     # the twelve channels-last planes
PLANES = slice(0, 13)            # the thirteen plane tensors: twelve planes and basis_mat.weight
LINEARS = slice(12, 31)          # every nn.Linear tensor of the list (the fragment cache is built from them)
RENDER_MLP = slice(13, 19)       # renderModule.mlp: (weight, bias) x 3; None under shadingMode=SH
WEIGHT_NET = slice(19, 31)       # vel_net.weight_net: (weight, bias) x 6; absent without use_vel

# ---- the 24 PDE tensors: the two halves
N_PDE = 24
PDE_WEIGHT_NET = slice(0, 12)
PDE_A_WEIGHT_NET = slice(12, 24)

# ---- struct member -> slots of the list, in the order of _lib.Grads._fields_ (a bare int: a scalar member)
RENDER_MEMBERS = (("dps", range(0, 3)), ("dpt", range(3, 6)), ("aps", range(6, 9)), ("apt", range(9, 12)), ("basis", 12),
                  ("rW", range(13, 19, 2)), ("rb", range(14, 19, 2)), ("vW", range(19, 31, 2)), ("vb", range(20, 31, 2)))
PDE_MEMBERS = (("vW", range(0, 12, 2)), ("vb", range(1, 12, 2)), ("aW", range(12, 24, 2)), ("ab", range(13, 24, 2)))
PDE_A_MEMBERS = PDE_MEMBERS[2:]  # the acceleration net alone: the only part of the 24-list an nvfi_field_desc takes from it


def at(group, tensors, total=N_RENDER):
    """a `total`-list of None with the slots of `group` holding `tensors`"""
    tensors = list(tensors)
    out = [None] * total
    if len(out[group]) != len(tensors):
        raise ValueError(f"{len(tensors)} tensors for the {len(out[group])} slots of {group}")
    out[group] = tensors
    return out


def fill(st, tensors, members=RENDER_MEMBERS, ptr=_lib.ptr):
    """Fill the pointer members of `st` (a FieldDesc or a Grads) from a list in slot order; a list that ends early leaves NULL behind it."""
    n = len(tensors)
    for name, slots in members:
        if isinstance(slots, int):
            setattr(st, name, ptr(tensors[slots]) if slots < n else None)
            continue
        arr = getattr(st, name)
        for i, k in enumerate(slots):
            arr[i] = ptr(tensors[k]) if k < n else None
    return st
