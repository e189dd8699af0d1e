"""Aged batches: the storage forms a long-running batch drifts into, planted into generated boards, and the header-flag
invariants every writer kernel must keep (gvec_device.hpp, "resident record layout" and "army storage").

  HF_WIDE        the env's armies live in the int32 escape block: exactly when one of them leaves [0, 65535]
  HF_LDIFF       the OwnedTiles planes are stored: exactly when some tile's listed player differs from its owner
  HF_SYNC        the player stats are what a stats pass over the lists and armies gives
  HF_FEWSPECIAL  2 * P + generals + cities <= W * H / 5

age_batch works on a VecEngine and an OracleBatch alike (game_state / read_state, write_state), a chunk of envs at a
time, and plants the same values into the same boards: twin batches stay twins."""
import numpy as np

import _harness as H
import _oracle as O

HF_DONE, HF_FOG, HF_WIDE, HF_SYNC, HF_FEWSPECIAL, HF_LDIFF = 1, 2, 4, 16, 64, 128
NARROW_MAX = 65535
# what age_batch plants, by env id % period (ids >= 4 of the period stay as they are)
EDGE, ESCAPE, HUGE, SATURATED = 0, 1, 2, 3
AGED_KINDS = 4


class _RawDeviceArray:
    """Zero-copy view of a raw device pointer for torch.as_tensor (the __cuda_array_interface__ protocol)."""

    def __init__(self, ptr, n_u32):
        self.__cuda_array_interface__ = {"shape": (n_u32,), "typestr": "<u4", "data": (int(ptr), False), "version": 2}


def header_flags(eng, env_begin=0, n=None):
    """Header dword H_DIMS >> 24 of envs [env_begin, env_begin + n), read through the zero-copy header buffer
    (GVEC_BUF_HEADER): only those envs' headers cross to the host."""
    import torch
    n = eng.B - env_begin if n is None else n
    eng.synchronize()
    t = torch.as_tensor(_RawDeviceArray(eng.device_buffer(0), eng.B * 24), device="cuda")
    h = t[env_begin * 24:(env_begin + n) * 24].cpu().numpy().view(np.uint32).reshape(n, 24)
    return h[:, 1] >> 24


def wide_envs(st):
    """envs holding an army outside [0, 65535]: the ones whose armies cannot be stored as u16 pairs"""
    a = st["army"]
    return ((a < 0) | (a > NARROW_MAX)).any(axis=1)


def desynced_envs(st):
    """envs in which some tile is owned by a player that does not list it (or listed by one that does not own it)"""
    return (st["listed"] != st["owner"]).any(axis=1)


def check_flag_invariants(eng, state, ctx="", env_begin=0):
    """state: the full game_state of envs [env_begin, env_begin + len) of `eng` (or the oracle's equal one)."""
    n = len(state["turn"])
    fl = header_flags(eng, env_begin, n)
    wide = wide_envs(state)
    bad = np.flatnonzero(((fl & HF_WIDE) != 0) != wide)
    assert len(bad) == 0, f"{ctx}: HF_WIDE <=> an army outside [0, 65535] fails in envs {bad[:8] + env_begin}"
    ldiff = desynced_envs(state)
    bad = np.flatnonzero(((fl & HF_LDIFF) != 0) != ldiff)
    assert len(bad) == 0, f"{ctx}: HF_LDIFF <=> listed != owner fails in envs {bad[:8] + env_begin}"
    typ, listed = state["type"], state["listed"]
    special = ((typ == 1) | (typ == 2)).sum(axis=1)
    few = 2 * state["players"].astype(np.int64) + special <= (state["width"].astype(np.int64) * state["height"]) // 5
    bad = np.flatnonzero(((fl & HF_FEWSPECIAL) != 0) != few)
    assert len(bad) == 0, f"{ctx}: HF_FEWSPECIAL <=> 2P + generals + cities <= N/5 fails in envs {bad[:8] + env_begin}"
    sync = np.flatnonzero(fl & HF_SYNC)
    if len(sync):
        P = state["army_count"].shape[1]
        a = state["army"][sync].astype(np.int64)
        for p in range(P):
            mine = listed[sync] == p
            tiles = mine.sum(axis=1)
            army = np.where(mine, a, 0).sum(axis=1)
            bt = np.flatnonzero(state["tile_count"][sync, p] != tiles)
            ba = np.flatnonzero(state["army_count"][sync, p].astype(np.int64) != army)
            assert len(bt) == 0, (f"{ctx}: HF_SYNC but player {p}'s tile_count is not its listed tiles in envs {sync[bt][:8] + env_begin}: "
                                  f"{state['tile_count'][sync[bt][:4], p]} vs {tiles[bt][:4]}")
            assert len(ba) == 0, (f"{ctx}: HF_SYNC but player {p}'s army_count is not its listed armies in envs {sync[ba][:8] + env_begin}: "
                                  f"{state['army_count'][sync[ba][:4], p]} vs {army[ba][:4]}")
    return fl


def _mix(seed, env, tile):
    """A counter hash (splitmix64's finaliser) of (seed, env, tile): the same draw for an env whatever chunk holds it."""
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.asarray(env, np.uint64) * np.uint64(0xBF58476D1CE4E5B9)
             + np.asarray(tile, np.uint64) * np.uint64(0x94D049BB133111EB))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def age_batch(target, seed, env_begin=0, n=None, period=AGED_KINDS + 2, turn_offsets=True, chunk=16384):
    """Plants the aged forms into envs [env_begin, env_begin + n) of a VecEngine or an OracleBatch, by env id % period:

      EDGE       generals and owned cities at 65,300 .. 65,535: production pushes them over (narrow -> wide)
      ESCAPE     one owned general at 65,536 .. 131,070: a half move brings it back to narrow (wide -> narrow)
      HUGE       every owned general at 10^6 .. 10^8 (a player's sum stays far below 2^31, generals_vec.h)
      SATURATED  every owned tile at 65,535: the largest per-lane sums the narrow (24-bit) stats path meets

    and, with turn_offsets, turn += env id % 25 on every env, so that the growth turns fall on different envs.
    The lists differing from ownership (HF_LDIFF) come from playing: a few turns with invalid_permille >= 50."""
    read = target.game_state if hasattr(target, "game_state") else target.read_state
    end = target.B if n is None else env_begin + n
    for lo in range(env_begin, end, chunk):
        m = min(chunk, end - lo)
        st = read(lo, m, fields=("army", "owner", "type", "turn"))
        ids = np.arange(lo, lo + m, dtype=np.int64)
        kind = ids % period
        army, owner, typ = st["army"].astype(np.int64), st["owner"], st["type"]
        r = _mix(seed, ids[:, None], np.arange(army.shape[1])[None, :])
        owned = owner >= 0
        gens = owned & (typ == 1)
        k = kind[:, None]
        edge = (k == EDGE) & owned & ((typ == 1) | (typ == 2))
        army = np.where(edge, 65300 + (r % np.uint64(236)).astype(np.int64), army)
        # ESCAPE: the owned general with the largest draw
        pick = np.where(gens, r, np.uint64(0))
        one = gens & (pick == pick.max(axis=1, keepdims=True)) & (k == ESCAPE)
        army = np.where(one, 65536 + (r % np.uint64(65535)).astype(np.int64), army)
        army = np.where((k == HUGE) & gens, 10 ** 6 + (r % np.uint64(99 * 10 ** 6)).astype(np.int64), army)
        army = np.where((k == SATURATED) & owned, NARROW_MAX, army)
        out = {"army": army.astype(np.int32)}
        if turn_offsets:
            out["turn"] = (st["turn"] + ids % 25).astype(np.int32)
        target.write_state(out, lo)


def aged_pair(g, mw, mh, maxp, sizes, seed, fog=True, warm=8, warm_permille=80, prod=(1, 1, 1), interval=25):
    """A VecEngine and an oracle dealt the same boards and pool, `warm` lock-step turns with invalid moves, then aged.
    g: the loaded package; None: the oracle alone, played and aged the same way (the engine returned is None).
    prod, interval: the production config of both."""
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, sizes, mw, mh)
    B = len(sizes)
    eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=fog, auto_reset=True, production=prod, normal_growth_interval=interval) if g is not None else None
    ora = O.OracleBatch(B, mw, mh, maxp, fog=fog, prod=prod, interval=interval)
    pool = min(16, B)
    for e in (eng, ora) if eng is not None else (ora,):
        e.reset(army, owner, typ, ws, hs, ps)
    ora.set_pool(pool, 70 + seed, ws[:pool], hs[:pool], ps[:pool])
    if eng is None:
        for _ in range(warm):
            ora.step(ora.agent_actions(seed, warm_permille))
        age_batch(ora, seed)
        return None, ora
    eng.build_board_pool(pool, 70 + seed, ws[:pool], hs[:pool], ps[:pool])
    H.run_lockstep(eng, ora, warm, seed, invalid_permille=warm_permille, check_every=warm, want_mask=False, ctx="warm-up")
    age_batch(eng, seed)
    age_batch(ora, seed)
    st = eng.game_state()
    H.assert_states_equal(st, ora.read_state(), "after aging")
    check_flag_invariants(eng, st, "write_state of the aged values")
    return eng, ora


class FormsTally:
    """Counts, over the states of a run, the envs in each form and the envs that changed form between two states."""

    def __init__(self):
        self.prev = None
        self.wide = self.ldiff = self.to_wide = self.to_narrow = 0

    def add(self, st):
        wide = wide_envs(st)
        self.wide += int(wide.sum())
        self.ldiff += int(desynced_envs(st).sum())
        if self.prev is not None:
            self.to_wide += int((wide & ~self.prev).sum())
            self.to_narrow += int((~wide & self.prev).sum())
        self.prev = wide

    def counts(self):
        return {"wide": self.wide, "ldiff": self.ldiff, "to_wide": self.to_wide, "to_narrow": self.to_narrow}

    def assert_all_seen(self, ctx=""):
        c = self.counts()
        assert all(v > 0 for v in c.values()), f"{ctx}: the run must contain wide and HF_LDIFF envs and both transitions: {c}"
