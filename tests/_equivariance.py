"""TEST INFRASTRUCTURE - the eight symmetries of the rectangle applied to everything the engine reads and writes: boards,
moves, whole states, packed masks, observations and stream deltas, in numpy.

The rules do not know which way the board is turned: step(g.s, g.a) = g.step(s, a) for every symmetry g, field for field.
This file builds g.s and g.a; the tests (test_equivariance_reference.py on the oracle, test_hip_equivariance.py on the
device) step a board and its images side by side, as separate envs of one padded batch, and compare.

It shares nothing with the kernels: a tile goes where tests/_symmetry_reference.map_xy sends its coordinates, a direction
where map_vector sends its vector, planes move by transform_planes.  The only index arithmetic here is the permutation
perm[t] = g(t) of an env's tiles, built from map_xy.  A transposing symmetry (sym & 4) swaps the env's width and height, so
at engine level, where every env carries its own dims, all eight apply to a non-square board too.

An env's tile row is [stride], the board's w * h tiles first (index y * w + x), padding behind them."""
import numpy as np

from _oracle import ACTION_DTYPE
from _symmetry_reference import map_vector, map_xy, transform_planes

TILE_FIELDS = ("army", "owner", "type", "visible", "listed", "changed", "vis_changed")
PAD = {"army": 0, "owner": -1, "type": 0, "visible": 0, "listed": -1, "changed": 0, "vis_changed": 0}
ENGINE_VECTORS = ((0, -1), (1, 0), (0, 1), (-1, 0))        # the engine's legal mask: up, right, down, left
SERIALIZER_VECTORS = ((0, -1), (0, 1), (-1, 0), (1, 0))    # the serializer's mask: up, down, left, right
ALL_SYMS = tuple(range(8))
FLIP_SYMS = (0, 1, 2, 3)                                   # the symmetries that keep width and height


def image_dims(w, h, sym):
    return (h, w) if sym & 4 else (w, h)


_PERMS = {}


def tile_perm(w, h, sym):
    """int64 [w * h]: perm[t] = g(t), the index tile t has on the image board"""
    perm = _PERMS.get((w, h, sym))
    if perm is None:
        t = np.arange(w * h, dtype=np.int64)
        gx, gy = map_xy(sym, t % w, t // w, w, h)
        perm = _PERMS[(w, h, sym)] = gy * image_dims(w, h, sym)[0] + gx
        perm.setflags(write=False)
    return perm


def image_tiles(row, w, h, sym, pad=0):
    """row [..., stride] -> out with out[..., g(t)] = row[..., t] for the board's tiles, `pad` behind them"""
    row = np.asarray(row)
    out = np.full_like(row, pad)
    out[..., tile_perm(w, h, sym)] = row[..., : w * h]
    return out


def orbit_boards(army, owner, typ, w, h, p, syms):
    """Boards [n][stride] with per-env dims, syms[e] = the symmetries env e is imaged under (0, the board itself, first).
    Returns (army, owner, type, w, h, p, base, sym) of the image envs, env e's images side by side in the order of syms[e]:
    base[i] is the row among the images that holds image i's own board (its sym 0), sym[i] the symmetry."""
    rows = {"army": [], "owner": [], "type": []}
    ws, hs, ps, base, sym_of = [], [], [], [], []
    for e in range(len(w)):
        assert syms[e][0] == 0
        first = len(ws)
        for s in syms[e]:
            for f, plane in (("army", army), ("owner", owner), ("type", typ)):
                rows[f].append(image_tiles(plane[e], int(w[e]), int(h[e]), s, PAD[f]))
            iw, ih = image_dims(int(w[e]), int(h[e]), s)
            ws.append(iw), hs.append(ih), ps.append(int(p[e])), base.append(first), sym_of.append(s)
    i32 = lambda v: np.array(v, np.int32)
    return (np.stack(rows["army"]).astype(np.int32), np.stack(rows["owner"]).astype(np.int8), np.stack(rows["type"]).astype(np.uint8),
            i32(ws), i32(hs), i32(ps), np.array(base, np.int64), np.array(sym_of, np.int64))


def image_state(state, e, sym):
    """The state env e of `state` (VecEngine.game_state / OracleBatch.read_state) has on the image board: a dict of that one
    env's fields.  Tile fields move with their tiles, general_idx goes through g, width and height follow the symmetry,
    every other env and player field stays."""
    w, h = int(state["width"][e]), int(state["height"][e])
    out = {}
    for f, a in state.items():
        if f in TILE_FIELDS:
            out[f] = image_tiles(a[e], w, h, sym, PAD[f])
        elif f == "general_idx":
            g = a[e].astype(np.int64)
            out[f] = np.where(g >= 0, tile_perm(w, h, sym)[np.clip(g, 0, w * h - 1)], g).astype(a.dtype)
        elif f not in ("width", "height"):
            out[f] = a[e].copy()
    iw, ih = image_dims(w, h, sym)
    if "width" in state:
        out["width"] = state["width"].dtype.type(iw)
    if "height" in state:
        out["height"] = state["height"].dtype.type(ih)
    return out


def env_state(state, e):
    return {f: a[e] for f, a in state.items()}


def assert_env_states_equal(got, want, ctx=""):
    """got / want: one env's fields (env_state / image_state).  Every field bit for bit; general_idx by the contract of
    _harness.assert_states_equal where a player lists two or more generals: SOME listed general of that player."""
    for f in want:
        if f == "general_idx":
            continue
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(np.asarray(got[f]) != np.asarray(want[f]))
            at = tuple(bad[0]) if bad.size else ()
            raise AssertionError(f"{ctx}: field '{f}' differs at {len(bad)} place(s); first {at}: got {np.asarray(got[f])[at]}, the image of "
                                 f"the base env has {np.asarray(want[f])[at]} (board {want.get('width')}x{want.get('height')}, turn {want.get('turn')})")
    if "general_idx" in want:
        for p, (g, v) in enumerate(zip(got["general_idx"], want["general_idx"])):
            mine = np.flatnonzero((want["listed"] == p) & (want["type"] == 1)) if "listed" in want else ()
            if len(mine) >= 2:
                assert g in mine, f"{ctx}: player {p}'s general_idx {g} is not one of its listed generals {mine}"
            else:
                assert g == v, f"{ctx}: player {p}'s general_idx is {g}, the image of the base env has {v}"


def image_actions(acts, w, h, sym):
    """ACTION_DTYPE [...] for a w x h board -> the same moves on the image board: `from` and `to` through map_xy, on or
    off the board alike (an invalid move stays invalid for the same reason); flags kept.  A slot that holds no move
    (GVEC_ACT_VALID clear) has no coordinates to map and is kept as it is."""
    acts = np.asarray(acts, ACTION_DTYPE)
    out = acts.copy()
    moves = (acts["flags"] & 1) != 0
    for a, b in (("from_x", "from_y"), ("to_x", "to_y")):
        gx, gy = map_xy(sym, acts[a].astype(np.int64), acts[b].astype(np.int64), w, h)
        out[a] = np.where(moves, gx, acts[a]).astype(np.int8)
        out[b] = np.where(moves, gy, acts[b]).astype(np.int8)
    return out


def image_packed_mask(bits, w, h, sym, vectors):
    """bits uint8 [..., mask_bytes]: four direction bit-planes of mask_bytes / 4 bytes, bit t (LSB first) of plane d the move
    from tile t along vectors[d].  -> the mask of the image board: bit g(t) of the plane of map_vector(vectors[d])."""
    bits = np.ascontiguousarray(bits, np.uint8)
    plane = bits.shape[-1] // 4
    u = np.unpackbits(bits.reshape(bits.shape[:-1] + (4, plane)), axis=-1, bitorder="little")      # [..., d, t]
    assert not u[..., w * h:].any(), "mask bits set behind the board's last tile"
    out = np.zeros_like(u)
    perm = tile_perm(w, h, sym)
    for d, v in enumerate(vectors):
        out[..., vectors.index(map_vector(sym, *v)), perm] = u[..., d, : w * h]
    return np.packbits(out, axis=-1, bitorder="little").reshape(bits.shape)


def image_observation(obs, w, h, sym):
    """A [..., 9, h, w] observation (the gym's), or a [..., 9 * stride] row with the serializer's [9, h, w] tensor at its
    front and zeros behind: every plane through transform_planes."""
    obs = np.asarray(obs)
    if obs.ndim >= 3 and obs.shape[-3:] == (9, h, w):
        return transform_planes(obs, sym)
    n = 9 * w * h
    assert not obs[..., n:].any(), "observation row not zero behind its [9, h, w] tensor"
    out = np.zeros_like(obs)
    out[..., :n] = transform_planes(obs[..., :n].reshape(obs.shape[:-1] + (9, h, w)), sym).reshape(obs.shape[:-1] + (n,))
    return out


def image_deltas(updates, count, w, h, sym):
    """One env's stream deltas (VecEngine.stream_deltas: updates uint64 [cap], count) -> the image env's, as a sorted array:
    an env's updates are a set (Go's map order is unspecified), keyed by the mapped tile in bits 0-15; the other bits
    (type, visible, fog, owner, army) stay."""
    u = np.asarray(updates, np.uint64)[: int(count)]
    tile = (u & np.uint64(0xFFFF)).astype(np.int64)
    assert (tile < w * h).all(), "a stream delta names a tile outside the board"
    moved = (u & ~np.uint64(0xFFFF)) | tile_perm(w, h, sym)[tile].astype(np.uint64)
    return np.sort(moved)


def packed_deltas(offset, updates, e):
    """env e's slice of VecEngine.stream_deltas_packed's stream, as (updates, count) for image_deltas"""
    mine = np.asarray(updates)[int(offset[e]): int(offset[e + 1])]
    return mine, len(mine)


def moves_share_a_tile(acts, players):
    """Whether two of the first `players` slots of one env's [P] actions hold moves that touch a common tile"""
    seen = []
    for a in acts[:players]:
        if a["flags"] & 1:
            mine = {(int(a["from_x"]), int(a["from_y"])), (int(a["to_x"]), int(a["to_y"]))}
            if any(mine & other for other in seen):
                return True
            seen.append(mine)
    return False
