"""The ordinary turn's quiet planes (GVEC_QUIET, gvec_device.hpp): on its straight-line path the per-turn step kernel

    stores the visibility planes only when the fog update changed them          fog on and V non-empty BEFORE the turn
    stores the ownership planes only when the turn changed an owner             V non-empty AFTER the turn
                                                                                (V = VisibilityChangedTiles)

and leaves in memory what it did not change.  That makes four classes of an ordinary env-turn, (V before, V after) empty
or not.  Every comparison below is bit for bit against the oracle after every turn, on the full state read back from device
memory, on the masks and on the error code: a plane left stale in memory fails on the next read.  The batches are those of
tests/test_hip_ordinary_turn.py; the first test holds them, on the oracle alone, to a floor in every class and to the two
facts the kernel's tests rest on.  (The same tests held a build that also fetched the visibility planes only on the turns
that update them; that half measured slower and is not in the code, DESIGN.md 4.1 "Quiet planes".)"""
import functools

import numpy as np
import pytest

import _harness as H
import _oracle as O
import _ordinary_turn as T
import _state_forms as F
from test_hip_ordinary_turn import VARIANTS, VARIANT_IDS, lockstep, variant_pair

FLOOR = 0.05   # of a carrier batch's ordinary env-turns, in each of the four classes
CLASS_NAMES = ("V empty -> empty", "V empty -> some", "V some -> empty", "V some -> some")


def carries_ordinary(maxp, slots, parity):
    """gvec_device.hpp ordturn_fits for the agent's kernels (the action-reading ones carry the path on a subset)"""
    odd = parity == "odd"
    return maxp <= 2 or (slots <= 10 if maxp <= 4 else (slots <= 2 and not (slots == 2 and odd)))


def carries_quiet(maxp, slots, parity):
    """gvec_device.hpp quiet_fits: the own / vis boundary of the staged block lies on a 16-byte chunk"""
    fd = 2 * slots - (1 if parity == "odd" else 0)
    return carries_ordinary(maxp, slots, parity) and (maxp * fd) % 4 == 0


CARRIERS = [v for v in VARIANTS if carries_ordinary(*v)]
CARRIER_IDS = [f"p{m}_slots{s}_{o}" for m, s, o in CARRIERS]


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


class Classes:
    """The ordinary env-turns of a run by class, and the turns on which the oracle itself breaks one of the two facts:
    an owner changes exactly when V is non-empty afterwards; an empty V before the turn leaves `visible` as it was."""

    def __init__(self):
        self.n = np.zeros((2, 2), np.int64)
        self.broke_own = self.broke_vis = 0

    def add(self, ord_live, before, after):
        v0 = before["vis_changed"].astype(bool).any(axis=1)
        v1 = after["vis_changed"].astype(bool).any(axis=1)
        for a in (0, 1):
            for b in (0, 1):
                self.n[a, b] += int((ord_live & (v0 == bool(a)) & (v1 == bool(b))).sum())
        owner_moved = (before["owner"] != after["owner"]).any(axis=1)
        sight_moved = (before["visible"] != after["visible"]).any(axis=1)
        self.broke_own += int((ord_live & (owner_moved != v1)).sum())
        self.broke_vis += int((ord_live & ~v0 & sight_moved).sum())

    def shares(self):
        return self.n.ravel() / max(1, int(self.n.sum()))

    def __str__(self):
        return " / ".join(f"{name} {100 * s:.1f} %" for name, s in zip(CLASS_NAMES, self.shares())) + f" of {int(self.n.sum())}"


def classed_lockstep(eng, ora, model, turns, seed, permille, ctx, tally=None, auto_reset=False, acts_of=None):
    """test_hip_ordinary_turn.lockstep a turn at a time, every ordinary env-turn counted into its class"""
    tally = Classes() if tally is None else tally
    for k in range(turns):
        before = model.prev
        o = T.ordinary(model.flags(), before) & ~before["done"].astype(bool)
        lockstep(eng, ora, model, 1, seed, permille, f"{ctx} [{k}]", acts_of=acts_of, auto_reset=auto_reset)
        tally.add(o, before, model.prev)
    return tally


def variant_run(g, maxp, slots, parity):
    eng, ora = variant_pair(g, maxp, slots, parity)
    return classed_lockstep(eng, ora, T.FlagModel(ora.read_state()), 60, 5, 20, f"<{maxp},{slots},{parity}>")


@functools.lru_cache(maxsize=None)
def oracle_alone(maxp, slots, parity):
    return variant_run(None, maxp, slots, parity)


# ---- 1. the batches, on the oracle alone (no GPU) -------------------------------------------------------------------------
@pytest.mark.parametrize("maxp,slots,parity", CARRIERS, ids=CARRIER_IDS)
def test_oracle_alone_every_class_is_under_test(maxp, slots, parity):
    """Every class holds at least 5 % of the batch's ordinary env-turns (a condition on the batch: another board seed if it
    fails, never a lower floor), and the oracle keeps both facts on every one of them."""
    c = oracle_alone(maxp, slots, parity)
    print(f"<{maxp},{slots},{parity}>: {c}")
    assert c.broke_own == 0, f"<{maxp},{slots},{parity}>: {c.broke_own} ordinary env-turns changed an owner without a tile in V, or the reverse"
    assert c.broke_vis == 0, f"<{maxp},{slots},{parity}>: {c.broke_vis} ordinary env-turns with an empty V changed `visible`"
    assert c.shares().min() >= FLOOR, f"<{maxp},{slots},{parity}>: {c}"


# ---- 2. gvec_step from turn 0 ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_lockstep_from_turn_zero_on_every_variant(g, maxp, slots, parity):
    """60 turns with 20 permille of unchecked moves: envs cross between the general and the ordinary turn and between the
    four classes; where the variant carries the quiet planes every class was played."""
    c = variant_run(g, maxp, slots, parity)
    if carries_quiet(maxp, slots, parity):
        assert c.n.min() > 0, f"<{maxp},{slots},{parity}>: {c}"


# ---- 3. the agent's kernels, one launch a turn ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_agent_per_turn_against_the_oracle_on_every_variant(g, maxp, slots, parity):
    """step_kernel<.., AGENT = true, ..> against the oracle's own agent, 40 turns from turn 0 with 20 permille of unchecked
    moves: the full state and the masks after every launch, the classes from the device's own header flags."""
    eng, ora = variant_pair(g, maxp, slots, parity)
    ctx = f"agent <{maxp},{slots},{parity}>"
    c = Classes()
    before = ora.read_state()
    for k in range(40):
        o = T.ordinary(F.header_flags(eng), before) & ~before["done"].astype(bool)
        eng.rollout(1, 11, 20, fused=False, want_stats=False)
        ora.rollout(1, 11, 20)
        after = ora.read_state()
        H.assert_states_equal(eng.game_state(), after, f"{ctx} after turn {k + 1}")
        assert np.array_equal(eng.legal_action_mask_bits(), ora.legal_mask()), f"{ctx} after turn {k + 1}: legal masks differ"
        c.add(o, before, after)
        before = after
    print(f"{ctx}: {c}")
    assert c.n.sum() > 0, f"{ctx}: no env-turn was ordinary"


# ---- 4. a batch of the benchmark's kind and age -----------------------------------------------------------------------------
def aged_benchmark_pair(g):
    """16 boards 20x20 4P, 1,000 turns old by the oracle's own agent, imported into the engine"""
    B, w, h, p = 16, 20, 20, 4
    army, owner, typ, ws, hs, ps = H.gen_boards(4100, [(w, h, p)] * B, w, h)
    ora = O.OracleBatch(B, w, h, p, fog=True)
    ora.reset(army, owner, typ, ws, hs, ps)
    ora.rollout(1000, 41, 0)
    st = ora.read_state()
    eng = None
    if g is not None:
        eng = g.VecEngine(B, w, h, p, fog_of_war=True)
        eng.reset(army, owner, typ, ws, hs, ps)
        eng.write_state({f: a for f, a in st.items() if f not in ("width", "height", "players")})   # those are the reset's
        H.assert_states_equal(eng.game_state(), st, "aged import")
    model = T.FlagModel(st)
    model.imported()
    return eng, ora, model


def aged_benchmark_run(g):
    eng, ora, model = aged_benchmark_pair(g)
    assert (model.prev["turn"] == 1000).all() and not model.prev["done"].all()
    return classed_lockstep(eng, ora, model, 40, 43, 0, "aged 20x20 4P")   # turn 1,025 grows


def test_oracle_alone_aged_batch_is_mostly_quiet():
    c = aged_benchmark_run(None)
    print(f"aged 20x20 4P: {c}")
    assert c.broke_own == 0 and c.broke_vis == 0
    assert c.shares()[0] > 0.60, f"aged 20x20 4P: {c}"


@pytest.mark.gpu
def test_lockstep_on_an_aged_benchmark_batch(g):
    """Most turns of an old board move neither plane: 40 of them in a row, across a growth turn, leave what the oracle leaves."""
    aged_benchmark_run(g)


# ---- 5. planes written by others between the turns --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp,slots,parity", [(4, 7, "odd"), (2, 2, "odd")], ids=["p4_slots7_odd", "p2_slots2_odd"])
def test_foreign_writers_between_turns(g, maxp, slots, parity):
    """write_state changes `visible`, and later an owner and its army, in envs whose V is empty - on device and oracle
    alike.  The turns after must neither lose what the writer left nor bring back what it replaced: the quiet turns store neither plane."""
    eng, ora = variant_pair(g, maxp, slots, parity)
    ctx = f"foreign <{maxp},{slots},{parity}>"
    model = T.FlagModel(ora.read_state())
    classed_lockstep(eng, ora, model, 12, 5, 0, ctx + " warm-up")

    def poke(make, what):
        st = ora.read_state()
        quiet = ~st["vis_changed"].astype(bool).any(axis=1) & ~st["done"].astype(bool)
        assert quiet.any(), f"{ctx}: {int(quiet.sum())} live envs with an empty V before the {what} write"
        out = make(st, np.flatnonzero(quiet))
        for e in (eng, ora):
            e.write_state(out)
        model.prev = ora.read_state()
        model.imported()
        H.assert_states_equal(eng.game_state(), model.prev, f"{ctx} after the {what} write")
        c = classed_lockstep(eng, ora, model, 10, 5, 0, f"{ctx} after the {what} write")
        assert c.n[0].sum() > 0, f"{ctx}: no ordinary turn with an empty V after the {what} write: {c}"

    def sight(st, envs):
        vis = st["visible"].copy()
        vis[envs, :5] ^= 1          # player 0's sight of the first five tiles of the top row, turned over
        return {"visible": vis}

    def owner(st, envs):
        own, lst, army = st["owner"].copy(), st["listed"].copy(), st["army"].copy()
        for e in envs:
            free = np.flatnonzero((st["type"][e] == 0) & (st["owner"][e] < 0) & (np.arange(own.shape[1]) < st["width"][e] * st["height"][e]))
            own[e, free[0]] = lst[e, free[0]] = int(np.flatnonzero(st["alive"][e])[0])   # a free tile to the first live player
            army[e, free[0]] = 9
        return {"owner": own, "listed": lst, "army": army}

    poke(sight, "visible")
    poke(owner, "owner")


# ---- 6. fog off: the visibility planes are never stored on the ordinary path ---------------------------------------------------------
@pytest.mark.gpu
def test_fog_off_lockstep(g):
    B, w, h, p = 8, 9, 9, 4   # <4,2,odd>
    army, owner, typ, ws, hs, ps = H.gen_boards(6100, [(w, h, p)] * B, w, h)
    eng, ora = g.VecEngine(B, w, h, p, fog_of_war=False), O.OracleBatch(B, w, h, p, fog=False)
    for e in (eng, ora):
        e.reset(army, owner, typ, ws, hs, ps)
    c = classed_lockstep(eng, ora, T.FlagModel(ora.read_state()), 30, 7, 20, "fog off <4,2,odd>")
    assert c.n.sum() > 0 and c.n[:, 1].sum() > 0 and c.n[:, 0].sum() > 0, f"fog off: {c}"


# ---- 7. the fused rollout keeps the general code ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("slots,parity", [(7, "odd"), (10, "even")], ids=["4x7", "4x10"])
def test_per_turn_and_fused_rollouts_agree(g, slots, parity):
    """step_kernel with the on-device agent and rollout_kernel (every plane loaded once, stored once) from the same
    boards, 50 turns with re-deals and unchecked moves: the same state, masks and header flags."""
    B, maxp = 64, 4
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    army, owner, typ, w, h, p = H.gen_boards(900 + slots, sizes, mw, mh)
    out = []
    for fused in (False, True):
        eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True)
        eng.reset(army, owner, typ, w, h, p)
        eng.build_board_pool(8, 17, w[:8], h[:8], p[:8])
        eng.rollout(50, 19, 20, fused=fused, want_stats=False)
        out.append((eng.game_state(), eng.legal_action_mask_bits(), F.header_flags(eng)))
    (s0, m0, f0), (s1, m1, f1) = out
    assert sorted(s0) == sorted(s1)
    for f in s0:
        assert np.array_equal(s0[f], s1[f]), f"<4,{slots}>: field '{f}' differs between the per-turn and the fused rollout"
    assert np.array_equal(m0, m1), f"<4,{slots}>: masks differ between the per-turn and the fused rollout"
    assert np.array_equal(f0, f1), f"<4,{slots}>: header flags differ between the per-turn and the fused rollout"
