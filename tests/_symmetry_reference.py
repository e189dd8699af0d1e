"""The board symmetries of include/generals_vec.h "board symmetries" in numpy, written without the kernel's index arithmetic:
planes move by np.flip / np.swapaxes, action-indexed rows as [H, W, 5] arrays whose direction axis is permuted, an action by
where its own index lands, and the exactness of a half move is read off tests/_gym_reference.decode_actions."""
import functools

import numpy as np

import _gym_reference as G

# d -> d' per sym, as the header states them
DIR_TABLES = ((0, 1, 2, 3), (0, 3, 2, 1), (2, 1, 0, 3), (2, 3, 0, 1), (3, 2, 1, 0), (3, 0, 1, 2), (1, 2, 3, 0), (1, 0, 3, 2))
INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)


def num_symmetries(H, W):
    return 8 if H == W else 4


def map_xy(sym, x, y, W, H):
    """g(x, y): the three steps of the definition, on coordinates (on or off the board)"""
    if sym & 1:
        x = W - 1 - x
    if sym & 2:
        y = H - 1 - y
    return (y, x) if sym & 4 else (x, y)


def map_vector(sym, dx, dy):
    """a direction vector through the same three steps"""
    if sym & 1:
        dx = -dx
    if sym & 2:
        dy = -dy
    return (dy, dx) if sym & 4 else (dx, dy)


def transform_planes(x, sym):
    """x [..., H, W] -> out with out[g(t)] = in[t]"""
    if sym & 1:
        x = np.flip(x, -1)
    if sym & 2:
        x = np.flip(x, -2)
    if sym & 4:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def transform_action_rows(x, sym, H, W):
    """x [..., 5 * H * W] -> out with out[5 g(t) + d'] = in[5 t + d]"""
    b = np.asarray(x).reshape(x.shape[:-1] + (H, W, 5))
    if sym & 1:
        b = np.flip(b, -2)
    if sym & 2:
        b = np.flip(b, -3)
    if sym & 4:
        b = np.swapaxes(b, -2, -3)
    out = np.empty_like(b)
    out[..., list(DIR_TABLES[sym]) + [4]] = b
    return out.reshape(x.shape)


@functools.lru_cache(maxsize=None)
def _action_images(sym, H, W):
    """int64 [A]: where each action index lands"""
    A = 5 * H * W
    moved = transform_action_rows(np.arange(A, dtype=np.int64), sym, H, W)      # moved[a'] = a
    images = np.empty(A, np.int64)
    images[moved] = np.arange(A)
    return images


def transform_actions(a, sym, H, W):
    """a int64 [...] under one sym; actions outside [0, 5 H W) stay as they are"""
    a = np.asarray(a, np.int64)
    inside = (a >= 0) & (a < 5 * H * W)
    return np.where(inside, _action_images(sym, H, W)[np.where(inside, a, 0)], a)


@functools.lru_cache(maxsize=None)
def exact_tiles(sym, H, W):
    """bool [H * W]: the half move from tile t, as GeneralsEnv plays it, is moved by sym onto the half move from g(t)"""
    t = np.arange(H * W, dtype=np.int64)
    fx, fy, tx, ty, half, _ = G.decode_actions(5 * t + 4, W, H)
    assert half.all()
    gx, gy = map_xy(sym, fx, fy, W, H)
    gw = W                                              # sym & 4 only where W == H
    _, _, tx2, ty2, _, _ = G.decode_actions(5 * (gy * gw + gx) + 4, W, H)
    ex, ey = map_xy(sym, tx, ty, W, H)
    return (tx2 == ex) & (ty2 == ey)


def applied_symmetries(sym, action, H, W):
    """uint8 [rows]: sym, or 0 where sym is no symmetry of the board or the action is a half move that is not exact"""
    sym = np.asarray(sym, np.uint8).copy()
    sym[sym >= num_symmetries(H, W)] = 0
    if action is not None:
        action = np.asarray(action, np.int64)
        for r in range(sym.shape[0]):
            a = int(action[r])
            if 0 <= a < 5 * H * W and a % 5 == 4 and not exact_tiles(int(sym[r]), H, W)[a // 5]:
                sym[r] = 0
    return sym


def apply(sym, H, W, planes=(), mask=None, values=None, action=None, inverse=False):
    """The whole call on flat rows: sym [rows], planes a sequence of [rows, P, H, W], mask / values [rows, 5 H W], action
    [rows].  Returns (list of transformed plane sets, mask, values, action, applied)."""
    applied = applied_symmetries(sym, action, H, W)
    eff = np.array([INVERSE[s] for s in applied], np.uint8) if inverse else applied
    out_planes = [np.empty_like(p) for p in planes]
    out_mask = None if mask is None else np.empty_like(mask)
    out_values = None if values is None else np.empty_like(values)
    out_action = None if action is None else np.empty_like(np.asarray(action, np.int64))
    for e in range(8):
        rows = np.nonzero(eff == e)[0]
        if rows.size == 0:
            continue
        for src, dst in zip(planes, out_planes):
            dst[rows] = transform_planes(src[rows], e)
        if mask is not None:
            out_mask[rows] = transform_action_rows(mask[rows], e, H, W)
        if values is not None:
            out_values[rows] = transform_action_rows(values[rows], e, H, W)
        if action is not None:
            out_action[rows] = transform_actions(np.asarray(action, np.int64)[rows], e, H, W)
    return out_planes, out_mask, out_values, out_action, applied
