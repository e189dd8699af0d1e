"""What the configured-reward tests share - TEST INFRASTRUCTURE ONLY: the configs, the comparison of one call with the numpy
restatement (tests/_reward_reference.py), and the run every compiled variant is held to (tests/test_hip_reward_variants.py):
the oracle playing an aged ragged batch, with the events of the run counted from the restatement's own terms, so that the
floors asserted on the device are properties of the oracle run and can be kept without a device."""
import numpy as np

import _harness as H
import _reward_reference as R
import _state_forms as F

STATE = ("owner", "army", "type", "alive", "players", "width", "height", "turn")
VARIANT_B, VARIANT_TURNS = 54, 60
# seat subsets per handle limit; where every seat is asked for, once more as a bit mask
SUBSETS = {8: ([7], [0], [1, 2, 5, 7], [0, 2, 4, 6], 0xFF), 4: ([3], [0], [1, 3], [0, 1, 2]), 2: ([1], [0])}


def configs(C):
    """C: the package's RewardConfig"""
    return {"go_default": C.go_default(),
            "awkward": C(win_game=0.3, lose_game=-0.7, capture_city=1e-3, lose_city=-2.5, capture_general=0.123, lose_general=-3.3,
                         territory_gained=0.3, territory_lost=-0.3, army_gained=-0.7, army_lost=0.7, army_advantage=1e-3),
            "clip": C(capture_city=3.0, lose_city=-3.0, capture_general=5.0, lose_general=-5.0, territory_gained=0.5, territory_lost=-0.5,
                      invalid_action=-0.25, clip=True)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def seat_ids(players, max_p):
    """seat ids, ascending, of an id list or a bit mask"""
    if isinstance(players, int):
        return [p for p in range(max_p) if players >> p & 1]
    return sorted(players)


def assert_equals_restatement(got, prev, cur, cfg, invalid, ctx, want=None):
    """got = (rewards, done, terms) of one call for all seats: value for value the restatement, and the rewards once more as
    the terms recombined in the definition's order and put through the three rules (clip, no predecessor, invalid_action).
    want: reward_reference(prev, cur, cfg, invalid=invalid) where the caller has it already."""
    r, d, t = got
    wr, wt, wd = R.reward_reference(prev, cur, cfg, invalid=invalid) if want is None else want
    assert np.array_equal(bits(r), bits(wr)), (ctx, np.argwhere(bits(r) != bits(wr))[:4], r[bits(r) != bits(wr)][:4], wr[bits(r) != bits(wr)][:4])
    assert np.array_equal(t, wt), (ctx, np.argwhere(t != wt)[:4], t[t != wt][:4], wt[t != wt][:4])
    assert np.array_equal(d, wd), ctx
    P = r.shape[1]
    live = R.comparable_rows(prev, cur)[:, None] & (np.arange(P)[None] < cur["players"][:, None])
    raw = R.recombine(t, cfg)
    want = R.normalize_reward(raw) if cfg.clip else raw
    want = np.where(live, want, np.float32(0))
    if invalid is not None:
        want = np.where(invalid, want + np.float32(cfg.invalid_action), want)
    assert np.array_equal(bits(r), bits(want.astype(np.float32))), (ctx, "recombined")


class RunTally:
    """The events of a run, counted from the restatement's go_default terms of every turn."""
    PER_CASE = ("d_territory", "d_army", "cities_gained", "army_advantage", "wide_env_turns")
    PER_MAXP = ("cities_lost", "generals_gained", "generals_lost", "wins", "losses", "not_comparable", "resized")

    def __init__(self):
        self.c = dict.fromkeys(self.PER_CASE + self.PER_MAXP, 0)
        self.max_d_army = 0

    def add(self, prev, cur, terms):
        c, nz = self.c, (terms != 0).sum((0, 1))
        for name, j in (("d_territory", 0), ("d_army", 1), ("cities_gained", 2), ("cities_lost", 3), ("generals_gained", 4), ("generals_lost", 5),
                        ("army_advantage", 7)):
            c[name] += int(nz[j])
        c["wins"] += int((terms[..., 6] > 0).sum())
        c["losses"] += int((terms[..., 6] < 0).sum())
        c["wide_env_turns"] += int((cur["army"] > F.NARROW_MAX).any(1).sum())
        c["not_comparable"] += int((~R.comparable_rows(prev, cur)).sum())
        c["resized"] += int(((prev["width"] != cur["width"]) | (prev["height"] != cur["height"])).sum())
        self.max_d_army = max(self.max_d_army, int(np.abs(terms[..., 1].astype(np.int64)).max()))

    def assert_case_floors(self, ctx):
        short = [k for k in self.PER_CASE if self.c[k] < 1]
        assert not short, f"{ctx}: the run holds no {', '.join(short)}: {self.c}"

    def assert_maxp_floors(self, ctx):
        """what the cases of one handle limit must hold between them; the int -> float32 conversion of d_army rounds above 2^24"""
        short = [k for k in self.PER_MAXP if self.c[k] < 1]
        assert not short, f"{ctx}: the runs hold no {', '.join(short)}: {self.c}"
        assert self.max_d_army > 2 ** 24, f"{ctx}: the largest |d_army| is {self.max_d_army}"


def variant_case(g, maxp, slots, parity):
    """The aged ragged batch of one compiled variant, as test_per_turn_agent_step_on_aged_envs deals it -> (engine, oracle, seed,
    (max_w, max_h, per-env sizes)); g None: the oracle alone."""
    seed = 40 + slots
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, VARIANT_B)
    eng, ora = F.aged_pair(g, mw, mh, maxp, sizes, seed)
    return eng, ora, seed, (mw, mh, sizes)


def play_variant(ora, seed, cfg, before_step=None, after_step=None, turns=VARIANT_TURNS):
    """`turns` turns of the oracle's agent on `ora`.  before_step(k) comes after the state before the step was read;
    after_step(k, acts, err, prev, cur, want) after the oracle's step, want = reward_reference(prev, cur, cfg).  -> RunTally"""
    tally = RunTally()
    for k in range(turns):
        acts = ora.agent_actions(seed, 60 if k < 30 else 8)
        prev = ora.read_state(fields=STATE)
        if before_step is not None:
            before_step(k)
        err = ora.step(acts)
        cur = ora.read_state(fields=STATE)
        want = R.reward_reference(prev, cur, cfg)
        tally.add(prev, cur, want[1])
        if after_step is not None:
            after_step(k, acts, err, prev, cur, want)
    return tally


def resize_after_snapshot(targets, ora, batch, seed, begin):
    """The one sequence in which an env changes size while its turn counter goes UP after the snapshot.  (An env re-dealt by
    auto-reset starts again at turn 0, below any snapshot's turn, so there the turn rule alone already says "no predecessor".)
    Every one of `targets` (engines and the oracle alike) is dealt fresh boards at turn 0, begin() takes the snapshot, then
    every env is dealt the size of the env after it - two envs in three change size.  The caller plays one turn.
    -> (the oracle agent's moves for that turn, the state the snapshot was taken of)"""
    mw, mh, sizes = batch
    for e in targets:
        e.reset(*H.gen_boards(seed + 1, sizes, mw, mh))
    prev = ora.read_state(fields=STATE)
    begin()
    for e in targets:
        e.reset(*H.gen_boards(seed + 2, sizes[1:] + sizes[:1], mw, mh))
    return ora.agent_actions(seed, 8), prev


def resized_with_turn_up(prev, cur):
    """rows that only the snapshot's W | H << 8 keeps from being compared with an unrelated board"""
    return ((prev["width"] != cur["width"]) | (prev["height"] != cur["height"])) & (cur["turn"] > prev["turn"])
