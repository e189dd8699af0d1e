"""Production configs off the defaults, without a device (tests/_production_cases.py has the cases).

1. The oracle against the rule itself: with every action a no-op a turn is the count, production, stats and fog, and what
   production leaves has a closed form (production_manager.go:26-101, restated in numpy).  That makes the oracle a reference
   off the defaults independent of its own C code.
2. Reach: every (config, batch) the GPU tests run, played by the oracle alone, is what the case is for - the ordinary share,
   growth turns beside turns that do not grow, wide envs under the large rates, and every sum below 2^30 (the engine keeps
   armies and their sums as int32; the reference's 64-bit int has no such bound).  Conditions on the inputs, not tolerances.
3. The kernel's growth_turn arithmetic (gvec_packed.hpp), replayed in integers over every interval and turn below 65,536."""
import numpy as np
import pytest

import _harness as H
import _oracle as O
import _ordinary_turn as T
import _production_cases as PC
import _state_forms as F
import test_hip_ordinary_turn as OT

ALL = PC.CASES + PC.PLANTED
IDS = [c.id for c in ALL]
RUNS = ([(c, v) for c in PC.CASES for v in PC.THREE] + [(c, PC.PLANT_VARIANT) for c in PC.PLANTED]
        + [(c, v) for c in PC.CARRIERS for v in OT.VARIANTS if v not in PC.THREE])
RUN_IDS = [f"{c.id}-p{v[0]}_slots{v[1]}_{v[2]}" for c, v in RUNS]


# ---- 1. the oracle against the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_production_is_the_closed_form(case):
    _, ora = PC.case_pair(None, case, PC.PLANT_VARIANT)
    start = ora.read_state()
    assert not F.desynced_envs(start).any() and (start["alive"].sum(axis=1) == start["players"]).all()
    assert ((start["type"] == 2) & (start["owner"] >= 0)).any(axis=1).all(), "every env of a case batch owns a city on its first turn"
    nobody = np.zeros((ora.B, ora.max_p), O.ACTION_DTYPE)
    for k in range(1, min(case.turns, 50) + 1):
        assert not ora.step(nobody).any()
        st = ora.read_state()
        army, changed = PC.closed_form(start, case.prod, case.interval, k)
        assert np.array_equal(st["turn"], start["turn"] + k)
        assert np.array_equal(st["army"].astype(np.int64), army), f"{case.id}: armies after {k} turns"
        assert np.array_equal(st["changed"], changed), f"{case.id}: ChangedTiles after turn {k}"
        for f in ("owner", "listed", "type", "alive", "tile_count"):
            assert np.array_equal(st[f], start[f]), (case.id, k, f)
        for p in range(ora.max_p):
            assert np.array_equal(st["army_count"][:, p].astype(np.int64), np.where(st["listed"] == p, army, 0).sum(axis=1)), (case.id, k, p)


def test_closed_form_sees_each_rate():
    """the restatement itself on one hand-made row: a general, a city, a plain tile, a mountain, a neutral city, a dead player's tile"""
    st = {"type": np.array([[1, 2, 0, 3, 2, 0]], np.uint8), "listed": np.array([[0, 0, 0, -1, -1, 1]], np.int8),
          "alive": np.array([[1, 0]], np.uint8), "turn": np.array([4], np.int32), "army": np.array([[1, 2, 3, 0, 40, 9]], np.int32)}
    army, changed = PC.closed_form(st, (3, 2, 5), 3, 5)     # turns 5 .. 9: growth on 6 and 9
    assert army.tolist() == [[16, 12, 13, 0, 40, 9]] and changed.tolist() == [[1, 1, 1, 0, 0, 0]]
    army, changed = PC.closed_form(st, (0, 2, 5), 3, 4)     # turns 5 .. 8: growth on 6; turn 8 grows nothing, generals never
    assert army.tolist() == [[1, 10, 8, 0, 40, 9]] and changed.tolist() == [[0, 1, 0, 0, 0, 0]]


# ---- 2. reach -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant", RUNS, ids=RUN_IDS)
def test_oracle_alone_case_batch_is_what_the_case_is_for(case, variant):
    n_ord, n_live, reach, last = PC.oracle_run(case.id, variant)
    ctx = f"{case.id} {variant}: {n_ord} of {n_live} live env-turns ordinary, {reach.growth} growth env-turns, peak {reach.peak}"
    assert n_live == reach.live > 0
    assert reach.peak < PC.ARMY_BOUND, ctx
    share, want = n_ord / n_live, PC.SHARE_OF.get((case.id, variant), case.share)
    if want == "zero":
        assert n_ord == 0, ctx
    elif not PC.has_cities(variant) or variant not in PC.THREE + [PC.PLANT_VARIANT]:
        pass   # the carriers on the other variants: test_hip_ordinary_turn's own share test covers the batch under the defaults
    elif want == "band":
        assert OT.BAND[0] <= share <= OT.BAND[1], ctx
    elif want == "positive":
        assert n_ord > 0, ctx
    if case.interval == 1:
        assert reach.growth == n_live, ctx
    elif case.plant is None and case.turns < case.interval:
        assert reach.growth == 0, ctx    # the largest rate: the run ends at turn 8, before the sums reach 2^30 and before turn 25
    else:
        assert 0 < reach.growth < n_live, ctx
        for t in reach.growth_turns:     # a turn that does not grow beside every growth turn of the run
            assert {t - 1, t + 1} & reach.other_turns, (ctx, t)
    if max(case.prod) > F.NARROW_MAX:
        assert F.wide_envs(last).any(), ctx
    if case.plant is not None:
        assert min(reach.growth_turns) > case.plant and (case.interval != 25 or {65525, 65550} <= reach.growth_turns), (ctx, reach.growth_turns)


@pytest.mark.parametrize("case", PC.AGED_CASES, ids=[c.id for c in PC.AGED_CASES])
@pytest.mark.parametrize("aged", OT.AGED, ids=["4x7", "8x16"])
def test_oracle_alone_aged_case_batches(case, aged):
    (n_ord, n_live), reach = PC.aged_case_run(None, case, aged)
    ctx = f"aged {case.id} {aged}: {n_ord} of {n_live} ordinary, {reach.growth} growth env-turns, peak {reach.peak}"
    assert reach.peak < PC.ARMY_BOUND and n_live > 0, ctx
    if case.interval == 1:
        assert n_ord == 0 and reach.growth == n_live, ctx
    else:
        assert 0 < n_ord and 0 < reach.growth < n_live, ctx


@pytest.mark.parametrize("case,variant", [(c, v) for c in PC.CASES for v in PC.THREE], ids=[f"{c.id}-p{v[0]}_slots{v[1]}" for c in PC.CASES for v in PC.THREE])
def test_oracle_alone_rollout_sums_stay_below_the_bound(case, variant):
    """the fused-rollout comparison plays the same batches with the oracle's own agent"""
    _, ora = PC.case_pair(None, case, variant)
    ora.rollout(case.turns, PC.SEED, PC.PERMILLE)
    st = ora.read_state(fields=("army", "army_count"))
    assert 0 <= st["army"].min() and max(st["army"].max(), st["army_count"].max()) < PC.ARMY_BOUND, case.id


# ---- 3. growth_turn's integers ------------------------------------------------------------------------------------------------
def kernel_growth_turn(t, interval):
    """PBoard::growth_turn (gvec_packed.hpp) with the host's magic (gvec_api.hip base_args), on int64 arrays"""
    t, interval = np.asarray(t, np.int64), np.asarray(interval, np.int64)
    magic = ((2 ** 32 + interval - 1) // interval) & 0xFFFFFFFF
    q = (t * magic) >> 32
    r = (t - ((q * interval) & 0xFFFFFFFF) + 2 ** 31) % 2 ** 32 - 2 ** 31      # int32 wrap
    r = np.where(r < 0, r + interval, r)
    fast = (t < 0x10000) & (((interval - 2) & 0xFFFFFFFF) < 0xFFFE)
    return np.where(fast, r == 0, t % interval == 0)


def test_growth_turn_arithmetic_equals_the_remainder():
    """every interval below 65,536 at the turns where a wrong quotient shows - 0, the interval, its largest multiple below
    65,536, the neighbours of each, 65,535 - and 32 drawn turns; every turn below 65,536 for the intervals the cases use and
    their neighbours; the boundaries by hand.  (Interval 1 fails this on the magic alone: q = 0 for every t.)"""
    iv = np.arange(1, 0x10000, dtype=np.int64)[:, None]
    top = 0xFFFF // iv * iv
    t = np.concatenate([np.zeros_like(iv), iv - 1, iv, np.minimum(iv + 1, 0xFFFF), top - 1, top, np.minimum(top + 1, 0xFFFF), np.full_like(iv, 0xFFFF),
                        np.random.default_rng(1).integers(0, 0x10000, (len(iv), 32))], axis=1)
    assert np.array_equal(kernel_growth_turn(t, iv), t % iv == 0)
    t = np.arange(0x10000, dtype=np.int64)[None, :]
    iv = np.array([1, 2, 3, 4, 5, 7, 24, 25, 26, 255, 256, 257, 32767, 32768, 65534, 65535], np.int64)[:, None]
    assert np.array_equal(kernel_growth_turn(t, iv), t % iv == 0)
    for iv, ts in ((1, [0, 1, 2, 65535, 65536, 131070]), (65535, [65535, 65536, 131070]), (65536, [65535, 65536, 131072]), (25, [65525, 65536, 65550])):
        ts = np.array(ts, np.int64)
        assert np.array_equal(kernel_growth_turn(ts, iv), ts % iv == 0), iv
