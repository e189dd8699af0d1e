"""The hazard matrix on the oracle alone (no GPU): every (scenario, board, placement, seat map, army scale) that
tests/test_hip_hazard_matrix.py plays on the device is played here by OracleBatch and held to the facts tests/_hazards.py
derives from the Go rules; and the matrix itself is held to its coverage, so that dropping a case fails here.  None of the
coverage conditions is a measured number: they are counts over the cases the library builds."""
import functools

import numpy as np
import pytest

import _harness as H
import _hazards as Z
import _oracle as O
from test_hip_ordinary_turn import VARIANTS, VARIANT_IDS

# gvec_device.hpp ordturn_fits(agent = false): the action-reading step kernels that carry the ordinary path
CARRIERS = [(m, s, o) for m, s, o in VARIANTS if (s <= 7 if m <= 4 else s <= 1)]


@functools.lru_cache(maxsize=None)
def batch(maxp, slots, parity):
    return Z.Batch(maxp, slots, parity)


@functools.lru_cache(maxsize=None)
def played(maxp, slots, parity):
    """the batch played by the oracle, facts asserted on the way: which envs the flag model sends into the forced turn on the
    ordinary path"""
    return Z.play(batch(maxp, slots, parity))[0]


@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_oracle_holds_the_derived_facts(maxp, slots, parity):
    played(maxp, slots, parity)


def test_ten_by_ten_base_scale_matches_test_scenarios():
    """the nine scenarios of tests/test_scenarios.py, placed in a corner of its 10x10 board at base scale, on a handle of
    their own (a 10x10 handle is none of the variants' limits; the kernels it selects are <., 2, even>'s)"""
    cases = []
    for sc in Z.SCENARIOS[:9]:
        regime = sc.regimes[-1]
        got = Z.place(sc, "corner", 10, 10, sc.fillers(100, regime))
        assert got is not None and sc.regime_of(100, len(got[1])) == regime
        cases.append(Z.Case(sc, "corner", 10, 10, tuple(range(sc.roles)), Z.SCALES[0], regime, 0, *got))
    Z.play(Z.Batch.of_cases(3, "10x10", 10, 10, cases))


def all_cases():
    return [(v, c) for v in VARIANTS for c in batch(*v).cases]


def test_every_scenario_reaches_every_variant_it_can_be_seated_on():
    for v in VARIANTS:
        have = {c.sc.name for c in batch(*v).cases if (c.w, c.h) == H.VARIANT_DIMS[v[1:]]}
        want = {sc.name for sc in Z.SCENARIOS if sc.roles in Z.SEAT_MAPS[v[0]]}
        assert have == want, f"<{v}>: missing {sorted(want - have)}, unexpected {sorted(have - want)}"


# ---- the single-mover matrix of the kernels that take one learner seat ----------------------------------------------------
SINGLE = [sc for sc in Z.SCENARIOS if sc.single_mover]


@functools.lru_cache(maxsize=None)
def single_batch(maxp, slots, parity):
    return Z.Batch(maxp, slots, parity, mover_on_seat_0=True)


@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_every_single_mover_scenario_is_on_every_variant_with_its_mover_on_seat_0(maxp, slots, parity):
    """and the oracle holds the facts in the order of calls the GPU test makes: the forced turn with the generated envs
    sitting out (GVEC_ACT_SKIP_ENV), then one-turn rollouts of an agent that never moves"""
    b = single_batch(maxp, slots, parity)
    want = {sc.name for sc in SINGLE if sc.roles in Z.SEAT_MAPS[maxp]}
    assert len(want) == (4 if maxp == 2 else 6)
    assert {c.sc.name for c in b.cases} == want
    assert all(c.seats[0] == 0 and (c.w, c.h) == H.VARIANT_DIMS[(slots, parity)] for c in b.cases)
    for sc in SINGLE:
        mine = [c for c in b.cases if c.sc is sc]
        if mine:
            assert len({c.K.name for c in mine}) >= 2 and {"corner", "edges"} <= {c.kind for c in mine}, sc.name
            assert slots == 1 or any(Z.crossing(c) for c in mine), f"{sc.name} never crosses a boundary"
    nc, nobody = len(b.cases), np.zeros((b.B, maxp), O.ACTION_DTYPE)
    ora = O.OracleBatch(b.B, b.mw, b.mh, maxp, fog=True)
    ora.reset(b.army, b.owner, b.typ, b.w, b.h, b.p)
    ora.write_state(b.pokes(ora.read_state()))
    ora.step(nobody)
    ora.set_agent_mix(65536, 0)
    acts = b.actions(None, ora)
    for e, c in enumerate(b.cases):
        acts[e] = c.actions(0, maxp)
    acts["flags"][nc:, 0] = 4
    err, bits = ora.step(acts, want_mask=True)
    b.check_facts(0, ora.read_state(), err, bits)
    for t in range(1, Z.TURNS):
        ora.rollout(1, 9, 0)
        b.check_facts(t, ora.read_state(), np.zeros(b.B, np.int32), ora.legal_mask())


def test_single_mover_scales_and_regimes():
    cases = [c for v in VARIANTS for c in single_batch(*v).cases]
    for sc in SINGLE:
        mine = [c for c in cases if c.sc is sc]
        assert {c.K.name for c in mine} == {k.name for k in Z.SCALES} and {c.regime for c in mine} == set(sc.regimes), sc.name


def test_every_multi_slot_variant_is_crossed():
    both = set()
    for v in VARIANTS:
        if v[1] == 1:
            continue
        kinds = {Z.crossing(c) for c in batch(*v).cases} - {None}
        assert kinds, f"<{v}>: no capturing move crosses a 64-tile boundary"
        w = H.VARIANT_DIMS[v[1:]][0]
        assert "v" in kinds and (("h" in kinds) == (64 % w != 0 or any((64 * k) % w for k in range(1, v[1])))), f"<{v}>: crossings {kinds} on width {w}"
        for sc in Z.SCENARIOS:
            if sc.roles in Z.SEAT_MAPS[v[0]] and len(sc.groups) <= 4:
                assert any(Z.crossing(c) for c in batch(*v).cases if c.sc is sc), f"<{v}>: {sc.name} never crosses a boundary"
        both |= kinds
    assert both == {"h", "v"}


def test_placements_on_the_edges_and_transposed():
    for v in VARIANTS:
        cs = batch(*v).cases
        w, h = H.VARIANT_DIMS[v[1:]]
        assert any(c.kind == "corner" and c.idx(c.sc.groups[0][0][0]) == 0 for c in cs)
        last_row = [c for c in cs if c.kind == "edges" and all(c.cells[n][1] == h - 1 for n, _, _ in c.sc.groups[0][:2])]
        last_col = [c for c in last_row if all(c.cells[n][0] == w - 1 for n, _, _ in c.sc.groups[1])]
        assert last_row and last_col, f"<{v}>: nothing on the last row / column"
        if w != h:
            assert any(c.kind == "transposed" for c in cs)
        if (w, h) != Z.small_dims(w, h):
            assert any(c.kind == "small" and (c.w, c.h) == Z.small_dims(w, h) for c in cs), f"<{v}>: the ragged small board is unused"


def test_both_regimes_seat_maps_and_scales():
    cases = all_cases()
    for sc in Z.SCENARIOS:
        mine = [c for _, c in cases if c.sc is sc]
        assert {c.regime for c in mine} == set(sc.regimes), f"{sc.name}: regimes {set(c.regime for c in mine)}"
        assert {c.K.name for c in mine} == {k.name for k in Z.SCALES}, f"{sc.name}: scales"
        for maxp in (2, 4, 8):
            for seats in Z.SEAT_MAPS[maxp].get(sc.roles, []):
                assert any(v[0] == maxp and c.seats == seats for v, c in cases if c.sc is sc), f"{sc.name}: seat map {seats} of P{maxp} unused"
        # each regime on each player limit
        for maxp in (2, 4, 8):
            if sc.roles in Z.SEAT_MAPS[maxp]:
                assert {c.regime for v, c in cases if c.sc is sc and v[0] == maxp} == set(sc.regimes)
        for c in mine:
            assert sc.regime_of(c.w * c.h, len(c.filler_idx)) == c.regime, c.id
    assert {c.players for _, c in cases if c.sc.name == "capture_game_goes_on"} >= {3, 4, 8}
    assert all(c.turn0 % 25 + 2 + Z.TURNS < 25 for _, c in cases if c.sc.turn0 is None), "a case meets a growth turn"


@pytest.mark.parametrize("maxp,slots,parity", CARRIERS, ids=[f"p{m}_slots{s}_{o}" for m, s, o in CARRIERS])
def test_which_cases_enter_the_forced_turn_ordinary(maxp, slots, parity):
    """On the 18 action-reading carriers: exactly the narrow cases whose board has room for the predicate (P <= N / 10,
    2 P + generals + cities <= N / 5) enter the forced turn on the ordinary path - the warm-up pass put every one of them in
    sync - and, 5x5 apart (too many special tiles ever to be ordinary), some do."""
    b = batch(maxp, slots, parity)
    o = played(maxp, slots, parity)
    for e, c in enumerate(b.cases):
        n, special = c.w * c.h, sum(tl.type in (Z.G_, Z.C_) for tl in c.sc.tiles.values())
        narrow = c.K.name != "wide"
        want = narrow and not c.sc.unlisted and 10 * c.players <= n and 2 * c.players + special <= n // 5
        assert bool(o[e]) == want, f"{c.id}: ordinary = {bool(o[e])}, the predicate gives {want}"
    if (slots, parity) != (1, "odd"):
        assert o[:len(b.cases)].any(), "no case is ordinary on this carrier"
        assert not o[:len(b.cases)].all()


def test_a_turnover_above_the_threshold_is_played_from_the_ordinary_path():
    """capture_game_goes_on carries an unlisted tile (HF_LDIFF): never ordinary.  Its twin with matching lists is, in both
    regimes, on some carrier"""
    seen = set()
    for v in CARRIERS:
        o = played(*v)
        seen |= {c.regime for e, c in enumerate(batch(*v).cases) if c.sc.name == "capture_game_goes_on_lists_match" and o[e]}
    assert seen == {"below", "above"}
