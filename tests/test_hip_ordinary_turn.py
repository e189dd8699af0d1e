"""The per-turn step kernel's straight-line path for the ordinary turn (GVEC_ORDTURN, gvec_device.hpp): a wave decides once,
from its header words, whether its env is live, narrow, list-matched, in sync and on a non-growth turn
(PBoard::ordinary_turn; tests/_ordinary_turn.py restates it) and then plays an instantiation of the turn with those guards
folded.  Whichever path an env takes it must leave what the oracle leaves: the tests below run batches in which envs
cross between the two paths in both directions, force every event that leaves the straight line mid-turn, and hold the
per-turn kernel to the fused rollout, which keeps the general code."""
import numpy as np
import pytest

import _harness as H
import _oracle as O
import _ordinary_turn as T
import _state_forms as F

BAND = (0.25, 0.95)   # the ordinary share of env-turns a batch must have for BOTH paths to be under test
# board seeds per <players, slots, parity>: 300 + slots unless the oracle alone showed that batch outside the band
BOARD_SEEDS = {(8, 7, "even"): 309, (8, 7, "odd"): 308, (8, 10, "even"): 312, (8, 10, "odd"): 312, (8, 16, "even"): 316, (8, 16, "odd"): 317}
VARIANTS = [(maxp, slots, parity) for maxp in (2, 4, 8) for slots, parity in sorted(H.VARIANT_DIMS)]
VARIANT_IDS = [f"p{m}_slots{s}_{o}" for m, s, o in VARIANTS]
# aged batches: <players, slots, parity>, seed, unchecked moves per mille.  The eight-player batch on 32x32 heals its lists only
# on growth turns (a pass is full when a fifth of the board changed): with new aborts on top it stays below the band
AGED = [(4, 7, "odd", 57, 20), (8, 16, "even", 67, 0)]


# <*, 1, odd> (at most 32 tiles): H.VARIANT_DIMS gives it a 5x5 handle, on which 2 * 2 + two generals > 25 / 5 - HF_FEWSPECIAL
# cannot hold and no env is ever ordinary.  A 6x5 handle selects the same kernels, and a two-player board of 30 tiles without
# a city is ordinary (2 * 2 + 2 <= 6, 10 * 2 <= 30): the batch below is two such boards in three, the third a 5x5 one.
ONE_SLOT_ODD = (6, 5)


def without_cities(army, owner, typ):
    """the boards with every city turned into a plain, empty, unowned tile"""
    city = typ == 2
    return np.where(city, 0, army).astype(np.int32), np.where(city, -1, owner).astype(np.int8), np.where(city, 0, typ).astype(np.uint8)


def variant_boards(maxp, slots, parity, B, seed):
    """(max_w, max_h, boards) on the smallest boards that select the variant and can be ordinary"""
    if (slots, parity) == (1, "odd"):
        mw, mh = ONE_SLOT_ODD
        sizes = [((mw, mh) if i % 3 else (5, 5)) + (2,) for i in range(B)]
        army, owner, typ, w, h, p = H.gen_boards(seed, sizes, mw, mh)
        return mw, mh, without_cities(army, owner, typ) + (w, h, p)
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    return mw, mh, H.gen_boards(seed, sizes, mw, mh)


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def variant_pair(g, maxp, slots, parity, B=8, prod=(1, 1, 1), interval=25, seed=None, deal=None):
    """engine (None without g) and oracle on the smallest boards that select the variant, reset: turn 0.
    prod, interval: the production config of both; seed: another board seed; deal(army, owner, typ, w, h, p) -> the same six,
    changed before the reset (tests/_production_cases.py hands the cities out)"""
    seed = BOARD_SEEDS.get((maxp, slots, parity), 300 + slots) if seed is None else seed
    mw, mh, boards = variant_boards(maxp, slots, parity, B, seed)
    army, owner, typ, w, h, p = boards if deal is None else deal(*boards)
    eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, production=prod, normal_growth_interval=interval) if g is not None else None
    ora = O.OracleBatch(B, mw, mh, maxp, fog=True, prod=prod, interval=interval)
    for e in (eng, ora) if eng is not None else (ora,):
        e.reset(army, owner, typ, w, h, p)
    return eng, ora


def lockstep(eng, ora, model, turns, seed, permille, ctx, acts_of=None, auto_reset=False, prod=(1, 1, 1), interval=25, watch=None):
    """H.run_lockstep's loop, a turn at a time: error code, masks and the full state every turn, and before every turn the
    device's own header flags against the model's (tests/_ordinary_turn.py) - which envs take the ordinary path.
    eng None: the oracle alone.  prod, interval: the production config both were built with.  watch(before, after): called
    with the oracle's states around every turn.  Returns (ordinary env-turns, live env-turns)."""
    n_ord = n_live = 0
    for k in range(turns):
        live = ~model.prev["done"].astype(bool)
        o = T.ordinary(model.flags(), model.prev, interval=interval, prod=prod)
        if eng is not None:
            dev = T.ordinary(F.header_flags(eng), model.prev, interval=interval, prod=prod)
            assert np.array_equal(dev[live], o[live]), f"{ctx} turn {k}: the device's flags make envs {np.flatnonzero((dev != o) & live)[:8]} ordinary = {dev[(dev != o) & live][:8]}, the model says otherwise"
        n_ord, n_live = n_ord + int((o & live).sum()), n_live + int(live.sum())
        acts = ora.agent_actions(seed, permille) if acts_of is None else acts_of(k)
        oerr, obits = ora.step(acts, want_mask=True)
        st = ora.read_state()
        if eng is not None:
            herr, hbits = eng.step(acts, want_mask=True)
            assert np.array_equal(herr, oerr), f"{ctx} turn {k}: err differs in envs {np.flatnonzero(herr != oerr)[:8]}: hip={herr[herr != oerr][:8]} ora={oerr[herr != oerr][:8]}"
            assert np.array_equal(hbits, obits), f"{ctx} turn {k}: legal mask differs in envs {np.unique(np.argwhere(hbits != obits)[:, 0])[:8]}"
            H.assert_states_equal(eng.game_state(), st, f"{ctx} after turn {k + 1}")
        if watch is not None:
            watch(model.prev, st)
        model.step(oerr, st, auto_reset)
    return n_ord, n_live


def variant_run(g, maxp, slots, parity):
    eng, ora = variant_pair(g, maxp, slots, parity)
    st = ora.read_state()
    assert (st["turn"] == 0).all()
    return lockstep(eng, ora, T.FlagModel(st), 60, 5, 20, f"<{maxp},{slots},{parity}>")


def aged_run(g, maxp, slots, parity, seed, permille, prod=(1, 1, 1), interval=25, watch=None):
    B = 12
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = F.aged_pair(g, mw, mh, maxp, sizes, seed, prod=prod, interval=interval)
    st = ora.read_state()
    assert F.wide_envs(st).any() and F.desynced_envs(st).any(), "the aged batch holds neither form"
    model = T.FlagModel(st)
    model.imported()
    out = lockstep(eng, ora, model, 30, seed, permille, f"aged <{maxp},{slots},{parity}>", auto_reset=True, prod=prod, interval=interval, watch=watch)
    if eng is not None:
        F.check_flag_invariants(eng, eng.game_state(), f"aged <{maxp},{slots},{parity}>")
    return out


# ---- the predicate's share, on the oracle alone (no GPU) ----------------------------------------------------------------
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_oracle_alone_both_paths_are_under_test(maxp, slots, parity):
    """The lock-step batch of every variant, played by the oracle alone: the ordinary share of its live env-turns lies in the
    band, so the GPU run of the same batch puts both instantiations under test.  (A condition on the batch, not a tolerance.)"""
    n_ord, n_live = variant_run(None, maxp, slots, parity)
    assert BAND[0] <= n_ord / n_live <= BAND[1], f"<{maxp},{slots},{parity}>: {n_ord} of {n_live} live env-turns are ordinary"


@pytest.mark.parametrize("maxp,slots,parity,seed,permille", AGED, ids=["4x7", "8x16"])
def test_oracle_alone_aged_batches_settle_into_ordinary(maxp, slots, parity, seed, permille):
    n_ord, n_live = aged_run(None, maxp, slots, parity, seed, permille)
    assert BAND[0] <= n_ord / n_live <= BAND[1], f"aged <{maxp},{slots},{parity}>: {n_ord} of {n_live} live env-turns are ordinary"


# ---- lock-step runs -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_lockstep_from_turn_zero_on_every_variant(g, maxp, slots, parity):
    """60 turns from turn 0 with fog, masks and 20 permille of unchecked moves: aborted turns clear HF_SYNC and leave list
    planes behind, the passes after them heal both, turns 25 and 50 grow - every env moves between the general and the
    ordinary path in both directions."""
    variant_run(g, maxp, slots, parity)


@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity,seed,permille", AGED, ids=["4x7", "8x16"])
def test_lockstep_on_aged_batches(g, maxp, slots, parity, seed, permille):
    """Wide armies and desynced lists (tests/_state_forms.py) start on the general path and settle into the ordinary one."""
    aged_run(g, maxp, slots, parity, seed, permille)


# ---- every event that leaves the straight line mid-turn, forced by explicit actions --------------------------------------
COLLIDE, CAPTURE, ABORT, OVERFLOW, PLAIN = range(5)


def _neighbour(t, w, h, typ):
    """a plain tile next to t, and t itself"""
    x, y = t % w, t // w
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        if 0 <= x + dx < w and 0 <= y + dy < h and typ[(y + dy) * w + x + dx] == 0:
            return (y + dy) * w + x + dx
    return None


def _free_run(w, h, typ, owner, n):
    """n plain, unowned tiles side by side in one row"""
    for t in range(w * h - n + 1):
        if t % w <= w - n and all(typ[t + i] == 0 and owner[t + i] < 0 for i in range(n)):
            return [t + i for i in range(n)]
    raise AssertionError(f"no run of {n} free plain tiles")


def exit_scenarios(g, w, h, players, auto_reset, seed=40, cities=True):
    """B envs, scenario = env % 5 (CAPTURE envs are two-player games: the capture ends them).  Plays two agent turns, plants
    the scenario's tiles, plays one empty turn (the import cleared HF_SYNC: the stats pass of that turn restores it), then
    the forced turn and five agent turns after it.  Returns (which envs were ordinary before the forced turn, the state
    after it, its error codes)."""
    B = 10
    sizes = [(w, h, 2 if e % 5 == CAPTURE else players) for e in range(B)]
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, sizes, w, h)
    if not cities:
        army, owner, typ = without_cities(army, owner, typ)
    eng = g.VecEngine(B, w, h, players, fog_of_war=True, auto_reset=auto_reset) if g is not None else None
    ora = O.OracleBatch(B, w, h, players, fog=True)
    for e in (eng, ora) if eng is not None else (ora,):
        e.reset(army, owner, typ, ws, hs, ps)
    if auto_reset:
        ora.set_pool(4, 77, ws[:4], hs[:4], ps[:4])
        if eng is not None:
            eng.build_board_pool(4, 77, ws[:4], hs[:4], ps[:4])
    model = T.FlagModel(ora.read_state())
    ctx = f"exits {w}x{h} auto_reset={auto_reset}"
    lockstep(eng, ora, model, 2, 3, 0, ctx + " warm-up", auto_reset=auto_reset)
    st = ora.read_state(fields=("army", "owner", "listed", "type"))
    forced = np.zeros((B, players), O.ACTION_DTYPE)

    def move(e, p, ft, tt):
        forced[e, p] = (ft % w, ft // w, tt % w, tt // w, 1, (0, 0, 0))

    for e in range(B):
        kind = e % 5
        ty, ow = st["type"][e], st["owner"][e]
        plant = {}
        if kind == CAPTURE:
            gen1 = int(np.flatnonzero((ty == 1) & (ow == 1))[0])
            t = _neighbour(gen1, w, h, ty)
            assert t is not None
            plant[t] = (0, 1000)
            move(e, 0, t, gen1)
        else:
            a, x, y = _free_run(w, h, ty, ow, 3)
            if kind == COLLIDE:      # both move onto the free tile between them: player 0 takes it, player 1 fails against it
                plant[a], plant[y] = (0, 10), (1, 7)
                move(e, 0, a, x)
                move(e, 1, y, x)
            elif kind == ABORT:      # player 0 moves an army that is player 1's
                plant[a] = (1, 5)
                move(e, 0, a, x)
            elif kind == OVERFLOW:   # 600 + 64,999 > 65,535: narrow at the load, wide at the store
                plant[a], plant[x] = (0, 65000), (0, 600)
                move(e, 0, a, x)
            else:
                plant[a] = (0, 10)
                move(e, 0, a, x)
        for t, (o, a) in plant.items():
            st["owner"][e, t] = st["listed"][e, t] = o
            st["army"][e, t] = a
    poke = {f: st[f] for f in ("army", "owner", "listed")}
    for e in (eng, ora) if eng is not None else (ora,):
        e.write_state(poke)
    model.prev = ora.read_state()
    model.imported()
    nobody = np.zeros((B, players), O.ACTION_DTYPE)
    lockstep(eng, ora, model, 1, 3, 0, ctx + " empty turn", acts_of=lambda k: nobody, auto_reset=auto_reset)
    flags = F.header_flags(eng) if eng is not None else model.flags()
    was_ordinary = T.ordinary(flags, model.prev)
    before = model.prev
    lockstep(eng, ora, model, 1, 3, 0, ctx + " forced turn", acts_of=lambda k: forced, auto_reset=auto_reset)
    after = model.prev
    kinds = np.arange(B) % 5
    assert (after["alive"].sum(axis=1) < before["alive"].sum(axis=1))[kinds == CAPTURE].all(), f"{ctx}: the capture eliminated nobody"
    assert after["done"][kinds == CAPTURE].all(), f"{ctx}: a two-player game survived the capture of a general"
    assert F.wide_envs(after)[kinds == OVERFLOW].all(), f"{ctx}: no army passed 65,535"
    assert (model.err != 0)[kinds == ABORT].all() and (model.err == 0)[kinds != ABORT].all(), f"{ctx}: error codes {model.err}"
    assert (after["turn"] == before["turn"] + 1).all()
    lockstep(eng, ora, model, 5, 3, 0, ctx + " turns after", auto_reset=auto_reset)
    return was_ordinary, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("auto_reset", [False, True], ids=["frozen", "redeal"])
@pytest.mark.parametrize("w,h,players", [(5, 5, 2), (6, 5, 2), (9, 9, 4)], ids=["5x5_p2", "6x5_p2", "9x9_p4"])
def test_every_mid_turn_exit(g, w, h, players, auto_reset):
    """Two moves on one tile, the capture of a general (elimination, turnover, and the end of a two-player game: the env is
    re-dealt or frozen in the launches after, beside ordinary envs), an aborting move and an army that outgrows u16, each
    against the oracle on the turn itself and the five after.  On 9x9 (<4,2,odd>) and on 6x5 without cities (<2,1,odd>)
    every env enters the forced turn on the ordinary path (read from the device's header flags); a 5x5 board has too many
    special tiles ever to be ordinary: there the same events run through the general code of <2,1,odd>."""
    was_ordinary, kinds = exit_scenarios(g, w, h, players, auto_reset, cities=(w, h) != (6, 5))
    if (w, h) != (5, 5):
        assert was_ordinary.all(), f"envs {np.flatnonzero(~was_ordinary)} entered the forced turn on the general path"
    else:
        assert not was_ordinary.any()


# ---- the fused rollout keeps the general code -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("slots,parity", [(7, "odd"), (10, "even")], ids=["4x7", "4x10"])
def test_per_turn_and_fused_rollouts_agree(g, slots, parity):
    """step_kernel with the on-device agent (ordinary and general turns) and rollout_kernel (general code only) from the
    same boards, 40 turns with re-deals and unchecked moves: the same state, the same masks."""
    B, maxp = 64, 4
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    army, owner, typ, w, h, p = H.gen_boards(700 + slots, sizes, mw, mh)
    out = []
    for fused in (False, True):
        eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True)
        eng.reset(army, owner, typ, w, h, p)
        eng.build_board_pool(8, 13, w[:8], h[:8], p[:8])
        eng.rollout(40, 9, 20, fused=fused, want_stats=False)
        out.append((eng.game_state(), eng.legal_action_mask_bits(), F.header_flags(eng)))
    (s0, m0, f0), (s1, m1, f1) = out
    assert sorted(s0) == sorted(s1)
    for f in s0:
        assert np.array_equal(s0[f], s1[f]), f"<4,{slots}>: field '{f}' differs between the per-turn and the fused rollout"
    assert np.array_equal(m0, m1), f"<4,{slots}>: masks differ between the per-turn and the fused rollout"
    assert np.array_equal(f0, f1), f"<4,{slots}>: header flags differ between the per-turn and the fused rollout"
    share = T.ordinary(f0, s0).mean()
    assert BAND[0] <= share, f"<4,{slots}>: only {share:.2f} of the envs would play their next turn on the ordinary path"


# ---- the agent's kernels, turn by turn against the oracle ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_agent_per_turn_against_the_oracle_on_every_variant(g, maxp, slots, parity):
    """step_kernel<.., AGENT = true, ..>, one launch a turn, against the oracle's own agent (OracleBatch.rollout draws the same
    moves): 40 turns from turn 0 with 20 permille of unchecked moves, the full state and the masks every turn.  The
    ordinary share is read from the device's header flags before every launch: where the variant carries the path
    (gvec_device.hpp ordturn_fits) that is the share of env-turns played on it."""
    eng, ora = variant_pair(g, maxp, slots, parity)
    ctx = f"agent <{maxp},{slots},{parity}>"
    n_ord = n_live = 0
    for k in range(40):
        st = ora.read_state(fields=("turn", "players", "width", "height", "done"))
        live = ~st["done"].astype(bool)
        o = T.ordinary(F.header_flags(eng), st)
        n_ord, n_live = n_ord + int((o & live).sum()), n_live + int(live.sum())
        eng.rollout(1, 9, 20, fused=False, want_stats=False)
        ora.rollout(1, 9, 20)
        H.assert_states_equal(eng.game_state(), ora.read_state(), f"{ctx} after turn {k + 1}")
        assert np.array_equal(eng.legal_action_mask_bits(), ora.legal_mask()), f"{ctx} after turn {k + 1}: legal masks differ"
    assert BAND[0] <= n_ord / n_live <= BAND[1], f"{ctx}: {n_ord} of {n_live} live env-turns were ordinary"
