"""The hazard matrix (tests/_hazards.py) on the device: one handle per variant, every scenario x placement a separate env
beside a few generated ones.  After every turn the facts derived from the Go rules, and error codes, packed legal masks and
the full game_state() bit for bit against the oracle's run of the same batch (tests/test_hazard_matrix.py holds that run to
the same facts without a GPU); check_flag_invariants after every board-writing launch."""
import numpy as np
import pytest

import _harness as H
import _hazards as Z
import _oracle as O
import _state_forms as F
from test_hazard_matrix import CARRIERS, batch, single_batch
from test_hip_ordinary_turn import VARIANTS, VARIANT_IDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def invariants(eng, st, ctx):
    F.check_flag_invariants(eng, st, ctx)


@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_step_kernel_on_every_action_reading_variant(g, maxp, slots, parity):
    """gvec_step: a warm-up empty turn (it sets HF_SYNC after the pokes), then the forced turn and five after it.  On the 18
    carriers of the ordinary path the device's own header flags send exactly the envs the CPU check names into the forced turn
    on that path (tests/test_hazard_matrix.py states which they are).  On the other 18 the same comparison only holds the
    flags to the model: that those kernels have the general code alone is gvec_device.hpp's ordturn_fits, restated in
    CARRIERS, and nothing this test can observe."""
    b = batch(maxp, slots, parity)
    eng = g.VecEngine(b.B, b.mw, b.mh, maxp, fog_of_war=True)
    model, dev = Z.play(b, eng, after_launch=invariants)
    n = len(b.cases)
    assert np.array_equal(dev[:n], model[:n]), f"the device's flags make cases {[b.cases[e].id for e in np.flatnonzero(dev[:n] != model[:n])][:6]} ordinary = {dev[:n][dev[:n] != model[:n]][:6]}"
    if (maxp, slots, parity) in CARRIERS and (slots, parity) != (1, "odd"):
        assert dev[:n].any()


@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_clones_play_the_forced_turn_like_their_source(g, maxp, slots, parity):
    """gvec_copy_envs of every case, after the warm-up, into a second handle in reversed order: the forced turn played there
    leaves what it leaves in the source, which the derived facts hold."""
    b = batch(maxp, slots, parity)
    src = g.VecEngine(b.B, b.mw, b.mh, maxp, fog_of_war=True)
    dst = g.VecEngine(b.B, b.mw, b.mh, maxp, fog_of_war=True)
    src.reset(b.army, b.owner, b.typ, b.w, b.h, b.p)
    dst.reset(b.army[::-1], b.owner[::-1], b.typ[::-1], b.w[::-1], b.h[::-1], b.p[::-1])
    src.write_state(b.pokes(src.game_state()))
    nobody = np.zeros((b.B, maxp), O.ACTION_DTYPE)
    src.step(nobody)
    perm = np.arange(b.B)[::-1].copy()
    dst.copy_envs(dst_ids=perm, src_ids=np.arange(b.B), src=src)
    st = dst.game_state()
    invariants(dst, st, "after copy_envs")
    assert np.array_equal(F.header_flags(dst)[perm], F.header_flags(src)), "the clone's header flags differ from its source's"
    acts, dacts = nobody.copy(), nobody.copy()
    for e, c in enumerate(b.cases):
        acts[e] = c.actions(0, maxp)
    dacts[perm] = acts
    serr, sbits = src.step(acts, want_mask=True)
    derr, dbits = dst.step(dacts, want_mask=True)
    s, d = src.game_state(), dst.game_state()
    invariants(dst, d, "clone after the forced turn")
    b.check_facts(0, s, serr, sbits)
    assert np.array_equal(derr[perm], serr) and np.array_equal(dbits[perm], sbits)
    for f in s:
        assert np.array_equal(d[f][perm], s[f]), f"clone: field '{f}' differs in envs {np.unique(np.argwhere(d[f][perm] != s[f])[:, 0])[:8]}"


# ---- gvec_gym_step_players: every seat a learner, every move the caller's, as gym action indices --------------------------
def gym_index(case, maxp, w):
    """[maxp] action indices of the forced turn: tile * 5 + direction, tile * 5 + 4 for a half move; -1 (refused: no move)
    for a seat without one.  None if the case's half move is not the one the index decodes to: a half move takes the first
    of (up, right, down, left) that stays on the board (tests/_gym_reference.py decode_actions)."""
    out = np.full(maxp, -1, np.int64)
    for role, s, d, move_all in case.sc.turns[0]:
        (fx, fy), (tx, ty) = case.cells[s], case.cells[d]
        k = {(0, -1): 0, (1, 0): 1, (0, 1): 2, (-1, 0): 3}[(tx - fx, ty - fy)]
        if not move_all:
            first = next(j for j, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0))) if 0 <= fx + dx < case.w and 0 <= fy + dy < case.h)
            if first != k:
                return None
        out[case.seats[role]] = (fy * w + fx) * 5 + (k if move_all else 4)
    return out


@pytest.mark.parametrize("maxp,slots,parity", [(2, 2, "odd"), (4, 4, "even"), (8, 7, "odd")], ids=["p2_9x10", "p4_16x16", "p8_20x20"])
def test_gym_step_players_with_every_seat_a_learner(g, maxp, slots, parity):
    """The full-size cases of the handle (the kernel's observations need one board size) with auto-reset and a board pool.
    alive, terminated, winner and the state go through the derived facts; needs_reset, invalid, error and the reward's sign
    are derived below; the state after the step and the re-deal of the games that ended are the oracle's."""
    import torch
    from generalsreinforcementlearning_amd._lib import check
    mw, mh = H.VARIANT_DIMS[(slots, parity)]
    idx = {}
    b = Z.Batch(maxp, slots, parity, only=lambda c: (c.w, c.h) == (mw, mh) and idx.setdefault(c.id, gym_index(c, maxp, mw)) is not None)
    assert (maxp == 2 or any(c.sc.half_move for c in b.cases)) and len(b.cases) > 20    # a half move needs the three-role scenario
    B, L, n, nc = b.B, maxp, mw * mh, len(b.cases)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
    ora = O.OracleBatch(B, mw, mh, maxp, fog=True)
    for x in (eng, ora):
        x.reset(b.army, b.owner, b.typ, b.w, b.h, b.p)
    eng.build_board_pool(4, 91)
    ora.set_pool(4, 91)
    poke = b.pokes(ora.read_state())
    nobody = np.zeros((B, maxp), O.ACTION_DTYPE)
    for x in (eng, ora):
        x.write_state(poke)
        x.step(nobody)
    st0 = ora.read_state()
    H.assert_states_equal(eng.game_state(), st0, "after the warm-up")
    bits, max_turns = (1 << maxp) - 1, 1000
    turn, resetting = z(B, torch.int64), z(B, torch.uint8)
    obs, mask = z((B, L, 9, n), torch.float32), z((B, L, n * 5), torch.uint8)
    out = {"reward": z((B, L), torch.float64), "invalid": z((B, L), torch.uint8), "error": z((B, L), torch.uint8), "alive": z((B, L), torch.uint8),
           "terminated": z(B, torch.uint8), "truncated": z(B, torch.uint8), "winner": z(B, torch.int8), "needs_reset": z(B, torch.uint8),
           "turn_out": z(B, torch.int64)}
    done0 = z(B, torch.uint8)
    check(eng.L.gvec_gym_observe_players(eng.h, bits, turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), out["reward"].data_ptr(),
                                         done0.data_ptr(), out["winner"].data_ptr()), "gvec_gym_observe_players")

    def step(acts, seed):
        ta = torch.from_numpy(np.ascontiguousarray(acts, np.int64)).cuda()
        o = out
        check(eng.L.gvec_gym_step_players(eng.h, bits, seed, ta.data_ptr(), resetting.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(),
                                          mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(), o["truncated"].data_ptr(),
                                          o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(), o["invalid"].data_ptr(),
                                          o["error"].data_ptr(), o["alive"].data_ptr()), "gvec_gym_step_players")
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in o.items()}

    acts = np.full((B, L), -1, np.int64)
    for e, c in enumerate(b.cases):
        acts[e] = idx[c.id]
    o = step(acts, 7)
    oerr, obits = ora.step(_case_actions(b), want_mask=True)
    hst, ost = eng.game_state(), ora.read_state()
    invariants(eng, hst, "gym players, forced turn")
    H.assert_states_equal(hst, ost, "gym players, forced turn")
    # the kernel's own outputs in the place of the state's fields, through the derived facts
    seen = dict(hst, alive=o["alive"], done=o["terminated"], winner=np.where(o["terminated"].astype(bool), o["winner"], -1).astype(np.int8))
    b.check_facts(0, seen, oerr, obits)
    assert np.array_equal(o["needs_reset"], o["terminated"]) and not o["truncated"].any()
    assert not o["terminated"][:nc].all() and (maxp == 2 or o["terminated"][:nc].any())    # no two-role scenario ends on the forced turn
    for e, c in enumerate(b.cases):
        was = st0["alive"][e].astype(bool)
        moved = acts[e] >= 0
        # every mover's index is a legal action of its view (its source is its own, lit, with more than one army): neither
        # invalid nor error; a seat alive at the start that sent -1 is invalid; a seat not alive then is not flagged
        assert np.array_equal(o["invalid"][e].astype(bool), was & ~moved), f"{c.id}: invalid {o['invalid'][e]}"
        assert not o["error"][e].any(), f"{c.id}: error {o['error'][e]}"
        assert set(c.sc.reward_sign) == set(range(c.sc.roles)), c.id
        for role, sign in c.sc.reward_sign.items():
            sign = sign(c.K) if callable(sign) else sign
            r = o["reward"][e, c.seats[role]]
            assert np.sign(r) == np.sign(sign), f"{c.id}: role {role}'s reward {r}, derived {sign}"
    # the next calls: the games that ended are re-dealt from the pool, the others play an empty turn (the abort after a
    # general fell ends its game only now: OVER runs a turn late)
    redealt = 0
    for call in (1, 2):
        ended = o["needs_reset"].astype(bool)
        resetting.copy_(torch.from_numpy(o["needs_reset"]).cuda())
        o = step(np.full((B, L), -1, np.int64), 7 + call)
        ora.step(nobody)
        hst, ost = eng.game_state(), ora.read_state()
        invariants(eng, hst, f"gym players, call {call} after")
        H.assert_states_equal(hst, ost, f"gym players, re-deal and empty turn, call {call} after")
        assert (hst["turn"][ended] == 0).all() and not o["terminated"][ended].any()
        redealt += int(ended[:nc].sum())
        if call == 1:
            b.check_facts(1, dict(hst, alive=o["alive"], done=o["terminated"],
                                  winner=np.where(o["terminated"].astype(bool), o["winner"], -1).astype(np.int8)), np.zeros(B, np.int32), eng.legal_action_mask_bits())
    assert redealt > 0


def _case_actions(b):
    acts = np.zeros((b.B, b.maxp), O.ACTION_DTYPE)
    for e, c in enumerate(b.cases):
        acts[e] = c.actions(0, b.maxp)
    return acts


# ---- the single-mover scenarios through the agent's kernels: every agent seat sits out -----------------------------------
@pytest.mark.parametrize("maxp,slots,parity", VARIANTS, ids=VARIANT_IDS)
def test_single_movers_through_gym_step_search_and_one_turn_rollouts(g, maxp, slots, parity):
    """gvec_set_agent_mix(65536, 0): the device's agent never moves.  The forced turn is gvec_gym_step's (the learner is seat
    0: the cases whose mover sits there, on the handle's full-size board) and, on a copy, a depth-1 gvec_search_playouts'
    with the move as the seat's candidate; the five turns after it are one-turn
    gvec_rollout(fused=False) launches - the AGENT = true instantiations playing empty turns."""
    import torch
    from generalsreinforcementlearning_amd._lib import check
    mw, mh = H.VARIANT_DIMS[(slots, parity)]
    b = single_batch(maxp, slots, parity)      # every single-mover scenario the handle seats (tests/test_hazard_matrix.py asserts it)
    B, n, nc = b.B, mw * mh, len(b.cases)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
    ora = O.OracleBatch(B, mw, mh, maxp, fog=True)
    for x in (eng, ora):
        x.reset(b.army, b.owner, b.typ, b.w, b.h, b.p)
    # gvec_gym_step asks for a pool; no single-mover scenario ends its game.  As many generals as the generator can space out
    pool = (np.full(4, mw, np.int32), np.full(4, mh, np.int32), np.full(4, min(maxp, max(2, n // 30)), np.int32))
    eng.build_board_pool(4, 91, *pool)
    ora.set_pool(4, 91, *pool)
    poke = b.pokes(ora.read_state())
    nobody = np.zeros((B, maxp), O.ACTION_DTYPE)
    for x in (eng, ora):
        x.write_state(poke)
        x.step(nobody)
        x.set_agent_mix(65536, 0)
    try:
        max_turns = 1000
        turn, resetting = z(B, torch.int64), z(B, torch.uint8)
        obs, mask = z((B, 9, n), torch.float32), z((B, n * 5), torch.uint8)
        o = {k: z(B, dt) for k, dt in (("reward", torch.float64), ("terminated", torch.uint8), ("truncated", torch.uint8), ("winner", torch.int8),
                                      ("needs_reset", torch.uint8), ("turn_out", torch.int64), ("played", torch.uint8), ("invalid", torch.uint8),
                                      ("error", torch.uint8))}
        done0 = z(B, torch.uint8)
        check(eng.L.gvec_gym_observe(eng.h, 0, turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), o["reward"].data_ptr(), done0.data_ptr(),
                                     o["winner"].data_ptr()), "gvec_gym_observe")
        acts = np.full(B, -1, np.int64)     # the generated envs: a refused action, the env sits the call out
        for e, c in enumerate(b.cases):
            acts[e] = gym_index(c, maxp, mw)[0]
        ta = torch.from_numpy(acts).cuda()
        # a depth-1 playout of the same move as the seat's only candidate, on a copy of the root: its score row is held to
        # the state the forced turn leaves, below
        from generalsreinforcementlearning_amd.search import PlayoutSearch
        terms = PlayoutSearch(eng, candidates=1, replicas=1, depth=1).evaluate(
            torch.arange(nc, dtype=torch.int32, device="cuda"), torch.zeros(nc, dtype=torch.int32, device="cuda"), ta[:nc].reshape(nc, 1).contiguous(), seed=5)
        terms = terms.cpu().numpy().reshape(nc, 8).astype(np.int64)
        check(eng.L.gvec_gym_step(eng.h, 0, 7, ta.data_ptr(), resetting.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(),
                                  o["reward"].data_ptr(), o["terminated"].data_ptr(), o["truncated"].data_ptr(), o["winner"].data_ptr(),
                                  o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(), o["played"].data_ptr(), o["invalid"].data_ptr(),
                                  o["error"].data_ptr()), "gvec_gym_step")
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in o.items()}
        oacts = _case_actions(b)
        oacts["flags"][nc:, 0] = 4          # GVEC_ACT_SKIP_ENV
        oerr, obits = ora.step(oacts, want_mask=True)
        hst = eng.game_state()
        invariants(eng, hst, "gym step, forced turn")
        H.assert_states_equal(hst, ora.read_state(), "gym step, forced turn")
        seen = dict(hst, done=o["terminated"], winner=np.where(o["terminated"].astype(bool), o["winner"], -1).astype(np.int8))
        b.check_facts(0, seen, oerr, obits)
        # valid, turns, alive, won, land, army, the other seats' land and army (search.py TERM_NAMES) of seat 0, from the state the
        # derived facts have just held
        tc, ac = hst["tile_count"][:nc].astype(np.int64), hst["army_count"][:nc].astype(np.int64)
        want = np.stack([np.ones(nc, np.int64), np.ones(nc, np.int64), hst["alive"][:nc, 0], (hst["done"][:nc] != 0) & (hst["winner"][:nc] == 0),
                         tc[:, 0], ac[:, 0], tc.sum(axis=1) - tc[:, 0], ac.sum(axis=1) - ac[:, 0]], axis=1)
        assert np.array_equal(terms, want), f"score rows differ in cases {[b.cases[e].id for e in np.flatnonzero((terms != want).any(axis=1))][:4]}"
        assert o["played"][:nc].all() and not o["played"][nc:].any() and not o["invalid"][:nc].any() and not o["error"][:nc].any()
        assert not o["terminated"].any() and not o["needs_reset"].any()      # no single-mover scenario ends its game
        for e, c in enumerate(b.cases):
            assert o["reward"][e] * c.sc.reward_sign[0] > 0, f"{c.id}: reward {o['reward'][e]}"
        for t in range(1, Z.TURNS):
            eng.rollout(1, 9, 0, fused=False, want_stats=False)
            ora.rollout(1, 9, 0)
            hst = eng.game_state()
            invariants(eng, hst, f"agent turn t={t}")
            H.assert_states_equal(hst, ora.read_state(), f"agent turn t={t}")
            bits = eng.legal_action_mask_bits()
            assert np.array_equal(bits, ora.legal_mask()), f"agent turn t={t}: legal masks differ"
            if t == 1:      # the generated envs sat the forced turn out: they are a turn behind from here on
                assert (hst["turn"][nc:] == 2).all()
            b.check_facts(t, hst, np.zeros(B, np.int32), bits)
    finally:
        eng.set_agent_mix()
