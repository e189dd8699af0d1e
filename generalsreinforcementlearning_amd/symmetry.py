"""symmetry — the eight symmetries of the board (four on a board that is not square), one per row of a batch: data
augmentation for replay samples, and group averaging of spatial Q values or logits (include/generals_vec.h "board
symmetries").

The game does not know left from right, so a stored transition (s, a, r, ns, d) is as good mirrored or turned.  One HIP launch
(gvec_obs_symmetry: one wavefront per row) on the current torch stream moves every tensor of a row with that row's own
symmetry; nothing synchronises with the host.

    s2, a2, ns2, applied = augment_transition(s, a, ns)                              # a replay batch, sym drawn per row
    obs2, mem2, mask2, act2 = apply_symmetry(sym, (obs, memory), mask=mask, action=act)
    (q,) = apply_symmetry(sym, values=net(obs2), inverse=True, height=H, width=W)    # Q values back in the original frame

sym in [0, 8): fx = sym & 1 mirrors x, fy = sym & 2 mirrors y, then tr = sym & 4 swaps x and y (square boards only).  A plane
moves as out[g(t)] = in[t]; a mask or a row of Q values as out[5 * g(t) + d'] = in[5 * t + d] with the direction permuted too;
an action as 5 * g(a // 5) + d'(a % 5).

The half move (a % 5 == 4) names no direction: the env plays the first of up, right, down, left that stays on the board, which
is not symmetric.  When `action` is given, a row whose action is a half move that the symmetry would turn into another move is
transformed with the identity instead - every tensor of it - and `applied` says which symmetry each row really got.
"""
import ctypes as C

from . import _obs_batch as ob
from ._lib import SYM_MAX_PLANE_SETS, ObsSymmetryArgs, check, load

MAX_PLANES = 64                            # per plane set
_INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)        # the two quarter turns are each other's inverse


def num_symmetries(height, width):
    """8 on a square board, else 4: the transpose needs width == height."""
    ob.check_board(int(width), int(height))
    return 8 if int(width) == int(height) else 4


def inverse_symmetry(sym):
    """The symmetry that undoes sym: an int in [0, 8), or an integer tensor of them (same dtype and device back)."""
    import torch
    if isinstance(sym, torch.Tensor):
        if sym.is_floating_point() or sym.dtype == torch.bool:
            raise TypeError(f"sym must be an integer tensor, not {sym.dtype}")
        return torch.tensor(_INVERSE, dtype=sym.dtype, device=sym.device)[sym.long()]
    if isinstance(sym, bool) or not isinstance(sym, int):
        raise TypeError(f"sym must be an int or a tensor, not {type(sym).__name__}")
    if not 0 <= sym < 8:
        raise ValueError(f"sym must be in [0, 8), not {sym}")
    return _INVERSE[sym]


def random_symmetries(shape, height, width, device, generator=None):
    """uint8 tensor of `shape` on `device`, uniform over the symmetries of a height x width board."""
    import torch
    return torch.randint(0, num_symmetries(height, width), tuple(shape), dtype=torch.uint8, device=device, generator=generator)


def _u8(mask):
    import torch
    mask = mask.detach().contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def apply_symmetry(sym, planes=(), mask=None, values=None, action=None, *, inverse=False, return_applied=False, height=None,
                   width=None):
    """Transforms every tensor given with the per-row symmetry `sym`; returns a tuple of new tensors in the order given
    (the plane sets, mask, values, action), then `applied` (uint8, sym's shape) with return_applied=True.

    sym     uint8 CUDA tensor [...], or an int for every row.  The values of a tensor are not checked here: a value that
            is no symmetry of the board (>= 8, or >= 4 where H != W) gives the identity and 0 in applied.
    planes  a float32 tensor [..., P, H, W], 1 <= P <= 64, or a tuple of up to four with the same leading shape and board
            (s and ns, memory planes, strategic features).  Read in place when the planes of a row are contiguous and the
            leading dimensions have one common stride, as for strategic_features; values are moved as bits.
    mask    bool or uint8 [..., 5 * H * W];  values float32 [..., 5 * H * W] (Q values, logits);  action int64 [...].
            An action outside [0, 5 * H * W) is copied unchanged.
    height, width  the board, needed when no planes are given.
    inverse  transform with each row's inverse symmetry.  The half-move rule is evaluated for sym itself either way, so with
            the same sym and the ORIGINAL action this undoes what the forward call did to planes, mask and values.
    The leading shape of every tensor is sym's (an int sym: that of the first tensor).  The results carry no autograd graph.
    ValueError / TypeError before any launch: non-tensors and wrong dtypes, CPU tensors or different devices, shapes that
    disagree, more than four plane sets, an int sym that the board does not have, nothing to transform."""
    import torch
    sets = (planes,) if isinstance(planes, torch.Tensor) else planes
    if not isinstance(sets, (tuple, list)):
        raise TypeError(f"planes must be a torch.Tensor or a tuple of them, not {type(planes).__name__}")
    sets = tuple(sets)
    if len(sets) > SYM_MAX_PLANE_SETS:
        raise ValueError(f"{len(sets)} plane sets: one call takes at most {SYM_MAX_PLANE_SETS}")
    if not sets and mask is None and values is None and action is None:
        raise ValueError("nothing to transform: no planes, mask, values or action")
    # the board and the leading shape, from the first plane set or from height= and width=
    lead = tuple(sym.shape) if isinstance(sym, torch.Tensor) else None
    H = W = None
    if (height is None) != (width is None):
        raise ValueError("height and width go together")
    if height is not None:
        H, W = int(height), int(width)
        ob.check_board(W, H)
    shaped = []
    for k, t in enumerate(sets):
        name = f"planes[{k}]"
        ob.check_tensor(t, name, (torch.float32,))
        t_lead, _, P, t_H, t_W = ob.read_plane_shape(t, name, MAX_PLANES)
        if H is None:
            H, W = t_H, t_W
        if (t_H, t_W) != (H, W):
            raise ValueError(f"{name} {tuple(t.shape)} is not on the {H}x{W} board of the call")
        lead = t_lead if lead is None else lead
        if t_lead != lead:
            raise ValueError(f"{name} {tuple(t.shape)} is not {lead + ('P', H, W)}")
        shaped.append(P)
    if H is None:
        raise ValueError("without planes the board is not known: give height= and width=")
    A = 5 * H * W
    for t, name, tail, dtypes in ((mask, "mask", (A,), (torch.bool, torch.uint8)), (values, "values", (A,), (torch.float32,)),
                                  (action, "action", (), (torch.int64,))):
        if t is None:
            continue
        ob.check_tensor(t, name, dtypes)
        if lead is None:
            lead = tuple(t.shape[:t.dim() - len(tail)])
        if tuple(t.shape) != lead + tail:
            raise ValueError(f"{name} {tuple(t.shape)} is not {lead + tail}")
    if isinstance(sym, torch.Tensor):
        ob.check_tensor(sym, "sym", (torch.uint8,))
    elif isinstance(sym, bool) or not isinstance(sym, int):
        raise TypeError(f"sym must be a uint8 tensor or an int, not {type(sym).__name__}")
    elif not 0 <= sym < num_symmetries(H, W):
        raise ValueError(f"sym {sym} is not one of the {num_symmetries(H, W)} symmetries of a {H}x{W} board")
    # the device last, so that a box without a GPU still sees every other refusal
    named = {f"planes[{k}]": t for k, t in enumerate(sets)}
    if isinstance(sym, torch.Tensor):
        named = {"sym": sym, **named}
    named.update(mask=mask, values=values, action=action)
    dev = ob.check_device("the symmetries are applied by a HIP kernel", next(iter(named)), **named)
    if dev is None:                                  # an int sym and nothing else cannot happen: something is transformed
        raise ValueError("nothing to transform: no planes, mask, values or action")
    if not isinstance(sym, torch.Tensor):
        sym = torch.full(lead, sym, dtype=torch.uint8, device=dev)
    rows = sym.numel()

    a = ObsSymmetryArgs(rows=rows, width=W, height=H, num_sets=len(sets), inverse=1 if inverse else 0, reserved=0)
    keep, results = [sym.detach().contiguous()], []
    a.sym = keep[0].data_ptr()
    for k, (t, P) in enumerate(zip(sets, shaped)):
        src, stride = ob.in_place_planes(t, 3, P, H, W)
        out = torch.empty(lead + (P, H, W), dtype=torch.float32, device=dev)
        keep.append(src)
        results.append(out)
        a.sets[k].in_, a.sets[k].out, a.sets[k].planes, a.sets[k].in_row_stride = src.data_ptr(), out.data_ptr(), P, stride
    if mask is not None:
        src = _u8(mask)
        out = torch.empty(lead + (A,), dtype=mask.dtype, device=dev)
        keep.append(src)
        results.append(out)
        a.mask_in, a.mask_out = src.data_ptr(), out.data_ptr()
    if values is not None:
        src = values.detach().contiguous()
        out = torch.empty(lead + (A,), dtype=torch.float32, device=dev)
        keep.append(src)
        results.append(out)
        a.values_in, a.values_out = src.data_ptr(), out.data_ptr()
    if action is not None:
        src = action.detach().contiguous()
        out = torch.empty(lead, dtype=torch.int64, device=dev)
        keep.append(src)
        results.append(out)
        a.action_in, a.action_out = src.data_ptr(), out.data_ptr()
    if return_applied:
        results.append(torch.empty(lead, dtype=torch.uint8, device=dev))
        a.applied = results[-1].data_ptr()
    if rows:
        check(load().gvec_obs_symmetry(dev.index, ob.stream(dev), C.byref(a)), "gvec_obs_symmetry")
    return tuple(results)


def augment_transition(s, a, ns, sym=None, generator=None):
    """(s', a', ns', applied) of a replay batch: s and ns float32 [..., P, H, W], a int64 [...], each row under its own
    symmetry - sym (uint8 [...], or an int) or, when None, one drawn per row from `generator`.  applied, uint8 [...], is the
    symmetry each row got: sym, or 0 where the action is a half move that sym would have turned into another move.  Rewards,
    done flags, discounts and priorities of the rows stay as they are; for an n-step sample `a` is the first action, which is
    all the sample holds.  Errors as for apply_symmetry."""
    import torch
    if sym is None:
        ob.check_tensor(s, "s", (torch.float32,))
        ob.check_tensor(a, "a", (torch.int64,))
        _, _, _, H, W = ob.read_plane_shape(s, "s", MAX_PLANES)
        sym = random_symmetries(a.shape, H, W, a.device, generator)
    s2, ns2, a2, applied = apply_symmetry(sym, (s, ns), action=a, return_applied=True)
    return s2, a2, ns2, applied
