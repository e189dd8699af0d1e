"""TEST INFRASTRUCTURE - which store code the observation and mask writers take, restated from their selectors.

The kernels that write into caller-owned device buffers pick their store path at run time from the address they are handed
and from the board's tile count.  Every selector below is a plain function of (address, stride or N, NSLOT) that returns the
paths one call of the device function takes as a list of (path, sh, windows): sh and windows are None unless the path
stores aligned 64-float (or 64-dword) windows, where sh is the destination's dword offset inside its 256-byte line and
windows the number of store windows that cover it.  A windowed call yields one entry per plane.

  site            device code                                  selector
  gym_emit.obs    gym_emit, observation planes                 ((obs >> 2) | stride) & 3, then NSLOT >= 7
  gym_emit.mask   gym_emit, mask bytes                         5 * stride & 15, mask & 15, & 3
  observe         observe_kernel                               ((out >> 2) | N) & 63, N the env's own tile count
  expand.tensor   expand_tensor (state and next_state)         ((out >> 2) | N) & 3, N the record's own tile count
  expand.mask     expand_records_kernel, action mask           (mk >> 2) & 63: one path, the window offset varies
  store_masks     store_masks_staged (gvec_step)               legal & 15 (of the handle's own buffer: see UNREACHABLE)
  query_masks     query_kernel (gvec_serializer_mask)          none: one path, run at every dword placement all the same

`*_launch` turn a launch's pointers and batch into the set of (site, path, sh, windows) over all its slots.  PLACEMENTS
are the byte offsets from a 256-byte-aligned base the tests put each buffer at; the selectors read no address bit above
the eighth, so the paths of a placement do not depend on where the allocator put the base."""
import numpy as np

import _harness as H

# byte offsets from a 256-byte-aligned base; never below the alignment the header gives the buffer's element
FLOAT_OFFSETS = (0, 4, 8, 12, 16, 252)      # float32 outputs, and the expanded action mask (4-byte aligned by the header)
BYTE_OFFSETS = (0, 1, 2, 3, 4, 16)          # uint8 masks
DWORD_OFFSETS = (0, 4, 8, 12)               # packed legal-mask buffers (4-byte aligned by the header)
BASE = 0x7F00_0000_0000                     # a stand-in for a 256-byte-aligned device address

_SLOT_LIMITS = ((64, 1), (128, 2), (256, 4), (448, 7), (640, 10), (1024, 16))   # gvec_dispatch.hpp


def nslot_of(stride):
    """the NSLOT of the kernel variant a handle of `stride` tiles runs"""
    return next(ns for limit, ns in _SLOT_LIMITS if stride <= limit)


def _windows(sh, n):
    """store windows k = 0, 1, ... with 64 k - sh < n: those that hold a tile"""
    return (n + sh + 63) // 64


def _planes(a0, pitch, n):
    """nine planes `pitch` dwords apart, each of n tiles, stored as aligned windows"""
    return [("windows", (a0 + c * pitch) & 63, _windows((a0 + c * pitch) & 63, n)) for c in range(9)]


# ---- the selectors, one per site -------------------------------------------------------------------------------------
def gym_obs(addr, stride, nslot):
    a0 = (addr >> 2) & 0xFFFFFFFF
    if (a0 | stride) & 3:
        return _planes(a0, stride, stride)
    return [("quads" if nslot >= 7 else "slots", None, None)]


def gym_mask(addr, stride, nslot=None):
    nbytes = 5 * stride
    if nbytes & 15 == 0 and addr & 15 == 0:
        return [("16-byte", None, None)]
    if nbytes & 3 == 0 and addr & 3 == 0:
        return [("4-byte", None, None)]
    return [("byte", None, None)]


def observe(addr, n, nslot=None):
    a0 = (addr >> 2) & 0xFFFFFFFF
    if (a0 | n) & 63:
        return _planes(a0, n, n)
    return [("slots", None, None)]


def expand_tensor(addr, n, nslot=None):
    a0 = (addr >> 2) & 0xFFFFFFFF
    if (a0 | n) & 3 == 0:
        return [("quads", None, None)]
    return _planes(a0, n, n)


def expand_mask(addr, stride, nslot=None):
    msh = (addr >> 2) & 63
    return [("windows", msh, _windows(msh, stride))]


def store_masks(addr, stride=None, nslot=None):
    return [("wide" if addr & 15 == 0 else "narrow", None, None)]


def query_masks(addr, stride=None, nslot=None):
    return [("narrow", None, None)]


SELECTORS = {"gym_emit.obs": (gym_obs, 4), "gym_emit.mask": (gym_mask, 1), "observe": (observe, 4), "expand.tensor": (expand_tensor, 4),
             "expand.mask": (expand_mask, 4), "store_masks": (store_masks, 4), "query_masks": (query_masks, 4)}


def reachable(site, n, nslot):
    """Everything the site can do for a buffer of `n` tiles per plane at ANY address its element's alignment allows:
    {(site, path, sh, windows)}.  (A selector reads no address bit above the eighth.)"""
    fn, elem = SELECTORS[site]
    return {(site,) + entry for off in range(0, 256, elem) for entry in fn(BASE + off, n, nslot)}


WINDOWED = ("gym_emit.obs", "observe", "expand.tensor", "expand.mask")
# store_masks_staged's narrow branch cannot be reached through the C ABI: gvec_step and the rollouts hand the kernel the
# handle's own resident mask buffer, which is 16-byte aligned and 16 * fd bytes per player, and copy it to the caller's
# array afterwards.  The caller's placement therefore exercises that copy; the selector is run on the resident buffer.
UNREACHABLE = {("store_masks", "narrow", None, None)}


def site_reach(site, stride, tiles, ns):
    """what the site can do on a batch at any legal address: observe / expand.tensor select on each env's own W * H"""
    sizes = sorted(set(tiles)) if site in ("observe", "expand.tensor") else [stride]
    return set().union(*(reachable(site, n, ns) for n in sizes)) - UNREACHABLE


def assert_coverage(got, stride, tiles):
    """got {site: {(site, path, sh, windows)}} runs every path each site has on this batch, every windowed path with
    sh = 0, 1, 63 (where the selector lets that sh reach it) and a value in between, and a full-slot board
    (stride == 64 * NSLOT) with the (NSLOT+1)-th window."""
    ns = nslot_of(stride)
    for site in SELECTORS:
        can = site_reach(site, stride, tiles, ns)
        assert got[site] <= can, (site, sorted(got[site] - can, key=str)[:4])
        assert {e[1] for e in got[site]} == {e[1] for e in can}, (site, "never runs", {e[1] for e in can} - {e[1] for e in got[site]})
        if site not in WINDOWED:
            continue
        can_sh = {e[2] for e in can if e[1] == "windows"}
        got_sh = {e[2] for e in got[site] if e[1] == "windows"}
        assert can_sh & {0, 1, 63} <= got_sh, (site, "window offsets never run", sorted(can_sh & {0, 1, 63} - got_sh))
        assert {1, 63} <= got_sh, site                       # within reach on every shape: the +4 and +252 byte placements
        assert any(1 < sh < 63 for sh in got_sh), site
        if 0 not in can_sh:   # no shift is out of the windowed path's reach only where it means another path altogether
            assert site != "expand.mask" and all(n % 4 == 0 for n in ([stride] if site == "gym_emit.obs" else tiles)), site
        if stride == 64 * ns:
            most = {e[3] for e in got[site] if e[1] == "windows"}
            assert ns + 1 in most, (site, "the (NSLOT+1)-th window never runs", most)
            if site == "gym_emit.obs":
                assert most == {ns + 1}                      # a full-slot board never shifts without it


# ---- launches ----------------------------------------------------------------------------------------------------------
def gym_launch(obs_ptr, mask_ptr, stride, slots):
    """a gym kernel writing `slots` = B * learners observations and masks"""
    ns, out = nslot_of(stride), set()
    for s in range(slots):
        out |= {("gym_emit.obs",) + e for e in gym_obs(obs_ptr + s * 36 * stride, stride, ns)}
        out |= {("gym_emit.mask",) + e for e in gym_mask(mask_ptr + s * 5 * stride, stride, ns)}
    return out


def observe_launch(out_ptr, stride, tiles, per_env):
    """gvec_observe: tiles[env] = the env's own W * H; per_env = 1 (one player) or max_players (player = -1)"""
    return {("observe",) + e for env, n in enumerate(tiles) for pl in range(per_env)
            for e in observe(out_ptr + (env * per_env + pl) * 36 * stride, n)}


def expand_launch(state_ptr, next_ptr, mask_ptr, stride, mp, slots):
    """gvec_expand_experience_records: slots = [(record, player, W * H of the record)] for the slots that hold an experience"""
    out = set()
    for rec, p, n in slots:
        s = rec * mp + p
        for ptr in (state_ptr, next_ptr):
            out |= {("expand.tensor",) + e for e in expand_tensor(ptr + s * 36 * stride, n)}
        out |= {("expand.mask",) + e for e in expand_mask(mask_ptr + s * 4 * stride, stride)}
    return out


def masks_launch(site, ptr):
    return {(site,) + e for e in SELECTORS[site][0](ptr)}


# ---- placements --------------------------------------------------------------------------------------------------------
def placements(*offset_lists):
    """Each buffer's offsets with the others at 0, then one placement with every buffer at its first offset that is below
    16 bytes and odd in units of its element (all odd together)."""
    k = len(offset_lists)
    out = [(0,) * k]
    for i, offs in enumerate(offset_lists):
        out += [tuple(o if j == i else 0 for j in range(k)) for o in offs if o]
    out.append(tuple(offs[1] if offs[1] != 1 else offs[3] for offs in offset_lists))    # 4 for dwords, 3 for bytes
    return out


GYM_PLACEMENTS = placements(FLOAT_OFFSETS, BYTE_OFFSETS)                       # (obs, mask)
OBSERVE_PLACEMENTS = [(o,) for o in FLOAT_OFFSETS]                             # (out,)
EXPAND_PLACEMENTS = placements(FLOAT_OFFSETS, FLOAT_OFFSETS, FLOAT_OFFSETS)    # (state, next_state, action_mask)
MASK_PLACEMENTS = [(o,) for o in DWORD_OFFSETS]                                # (legal_bits,)
B = 9                                                                          # envs of the GPU test's batch


def batch_tiles(maxp, slots, parity, batch=B):
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, batch)
    return mw * mh, [w * h for w, h, _ in sizes], [p for _, _, p in sizes]


def promised(maxp, slots, parity, learners, batch=B, acting=None):
    """{site: set of (site, path, sh, windows)} that the GPU test's launches reach on the variant's ragged batch, from the
    placements alone.  acting: the (record, player, W * H) slots of the recorded step that hold an experience (None: every
    env live and every seat of an env acting; which seats do act is up to the game)."""
    stride, tiles, players = batch_tiles(maxp, slots, parity, batch)
    out = {site: set() for site in SELECTORS}
    for obs, mask in GYM_PLACEMENTS:
        for L in (1, learners):
            for e in gym_launch(BASE + obs, BASE + mask, stride, batch * L):
                out[e[0]].add(e)
    for (o,) in OBSERVE_PLACEMENTS:
        for per_env in (1, maxp):
            out["observe"] |= observe_launch(BASE + o, stride, tiles, per_env)
    if acting is None:
        acting = [(rec, p, tiles[rec]) for rec in range(batch) for p in range(players[rec])]
    for st, nx, mk in EXPAND_PLACEMENTS:
        for e in expand_launch(BASE + st, BASE + nx, BASE + mk, stride, maxp, acting):
            out[e[0]].add(e)
    for (o,) in MASK_PLACEMENTS:
        out["store_masks"] |= masks_launch("store_masks", BASE)       # the handle's resident buffer, wherever the caller's is
        out["query_masks"] |= masks_launch("query_masks", BASE + o)
    return out


# ---- the state the GPU test launches on ---------------------------------------------------------------------------------
# Works on a VecEngine and on an OracleBatch alike (as tests/_state_forms.age_batch does), so the CPU test can hold the
# prepared state to what the GPU test needs of it without a device.
TURNS, MAX_TURNS = 30, 64
WIDE_ENV, MID_ENV = 1, 7          # largest board, every seat taken, for every player limit (variant_batch)
WIDE_ARMY, MID_ARMY = 70_000, 30_000


def _read(target):
    return target.game_state() if hasattr(target, "game_state") else target.read_state()


def _play(target, turns, seed):
    if hasattr(target, "game_state"):
        target.rollout(turns, seed, 0, fused=False, want_stats=False)
    else:
        target.rollout(turns, seed, 0)


def deal(target, maxp, slots, parity, seed):
    """the variant's ragged batch, dealt, with a pool of its own boards to re-deal from"""
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, target.B)
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, sizes, mw, mh)
    if not (typ[WIDE_ENV] == 3).any():
        # the generator gives a 5x5 board no mountain, and the mountain plane would be zeros: one plain neutral tile that
        # touches no general becomes one (a single mountain cannot cut a 5x5 board in two)
        gx, gy = np.divmod(np.flatnonzero(typ[WIDE_ENV] == 1), mw)[::-1]
        for t in np.flatnonzero((typ[WIDE_ENV][:mw * mh] == 0) & (owner[WIDE_ENV][:mw * mh] < 0)):
            if all(abs(t % mw - x) + abs(t // mw - y) > 1 for x, y in zip(gx, gy)):
                typ[WIDE_ENV][t] = 3
                break
    target.reset(army, owner, typ, ws, hs, ps)
    if hasattr(target, "game_state"):
        target.build_board_pool(target.B, 70 + seed, ws, hs, ps)
    else:
        target.set_pool(target.B, 70 + seed, ws, hs, ps)
    target.set_agent_mix(0, 0)       # every player with a legal move makes one: the recorded step has a slot for each


def plant(st):
    """What to write back into a played batch: every owned general of env WIDE_ENV above 65,535 and of env MID_ENV in
    1,000 .. 65,535 (each in its owner's sight), and in every 64-tile slot of env WIDE_ENV one neutral plain tile handed
    to a player who is alive, with an army and the 3x3 sight around it - so that no slot of the largest board is all zero
    in every observation."""
    army, owner, listed, visible = (st[k].copy() for k in ("army", "owner", "listed", "visible"))
    typ = st["type"]
    for env, base in ((WIDE_ENV, WIDE_ARMY), (MID_ENV, MID_ARMY)):
        gens = (typ[env] == 1) & (owner[env] >= 0)
        army[env][gens] = base + 1000 * owner[env][gens].astype(np.int32)
    e = WIDE_ENV
    w, h = int(st["width"][e]), int(st["height"][e])
    alive = [p for p in range(int(st["players"][e])) if st["alive"][e, p]]
    for s in range((w * h + 63) // 64):
        tiles = np.arange(64 * s, min(64 * s + 64, w * h))
        free = tiles[(typ[e][tiles] == 0) & (owner[e][tiles] < 0)]
        if not len(free) or not alive:
            continue
        # two neighbours in a row where the slot has them, for two different players: each sees a tile of the other's
        pairs = [int(t) for t in free if t + 1 in free and (t + 1) % w]
        first = pairs[len(pairs) // 2] if pairs else int(free[len(free) // 2])
        for k, t in enumerate([first, first + 1] if pairs else [first]):
            p = alive[(s + k) % len(alive)]
            owner[e, t] = listed[e, t] = p
            army[e, t] = 2 + s
            x, y = t % w, t // w
            for yy in range(max(0, y - 1), min(h, y + 2)):
                for xx in range(max(0, x - 1), min(w, x + 2)):
                    visible[e, yy * w + xx] |= np.uint8(1 << p)
    return {"army": army, "owner": owner, "listed": listed, "visible": visible}


def prepare(target, seed):
    """About TURNS turns of the on-device agent - a few more while an env sits on a finished game, which the next turn
    re-deals - then plant()."""
    _play(target, TURNS, seed)
    for _ in range(8):
        if not _read(target)["done"].any():
            break
        _play(target, 1, seed)
    target.write_state(plant(_read(target)))


def check_prepared(st, maxp, slots, parity):
    """what the GPU test's launches and their promised paths take for granted"""
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, len(st["turn"]))
    assert [(int(w), int(h), int(p)) for w, h, p in zip(st["width"], st["height"], st["players"])] == [tuple(s) for s in sizes], "a re-deal changed a size"
    assert not st["done"].any(), "an env sits on a finished game"
    for env in (WIDE_ENV, MID_ENV):
        assert sizes[env][:2] == (mw, mh) and sizes[env][2] == max(s[2] for s in sizes)   # (a small board seats fewer than maxp)
        assert st["alive"][env, 0] and st["alive"][env, sizes[env][2] - 1], f"seat 0 or the last seat of env {env} is out of the game"
    held = (st["owner"][WIDE_ENV] >= 0) & (st["army"][WIDE_ENV] > 0)
    assert all(held[64 * s:64 * s + 64].any() for s in range((mw * mh + 63) // 64)), "a 64-tile slot of the largest board holds no army"
    wide = (st["army"] > 65535).any(axis=1)
    assert wide[WIDE_ENV] and not wide[MID_ENV] and (st["army"][MID_ENV] >= 1000).any()
