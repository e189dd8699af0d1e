"""gvec_search_playouts_bot on the GPU: its terms against the CPU reference (tests/_search_bot_reference.py) exactly - the
roots whose playouts are won, lost and cut short, with and without fog and the exploration mix, every compiled variant, the
rare state forms - that with no seat on the rule it gives gvec_search_playouts' terms, that it reads its roots only, that it
equals the composition of existing calls on the device, that it repeats itself, and the Python front up to an Arena entrant."""
import ctypes as C

import numpy as np
import pytest

import _harness as H
import _oracle as O
import _search_bot_reference as SBR
import _search_reference as SR
import _state_forms as SF

pytestmark = pytest.mark.gpu


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _terms(eng, env_ids, players, cand, R, D, seed, bot_players, permille=0):
    """the kernel's terms [n, K, R, 8] on the host, through the Python front (bot_players: a bit mask, not 0)"""
    import generalsreinforcementlearning_amd as g
    cand = np.asarray(cand, np.int64)
    s = g.PlayoutSearch(eng, candidates=cand.shape[1], replicas=R, depth=D, rollout="bot", bot_players=bot_players, bot_random_permille=permille)
    assert s.bot_players == bot_players != 0
    out = s.evaluate(None if env_ids is None else _cuda(env_ids, np.int32), _cuda(players, np.int32), _cuda(cand, np.int64), seed)
    return out.cpu().numpy()


def _entry_point(eng, players, cand, R, D, seed, bot_players, permille=0, num_roots=None):
    """gvec_search_playouts_bot itself (the front calls the existing entry point when nothing is set) -> (rc, terms)"""
    import torch
    from generalsreinforcementlearning_amd import _lib as lib
    cand = np.asarray(cand, np.int64)
    n, K = cand.shape
    c, p = _cuda(cand, np.int64), _cuda(players, np.int32)
    terms = torch.full((n, K, R, 8), -7, dtype=torch.int32, device="cuda")
    a = lib.SearchArgs(num_roots=n if num_roots is None else num_roots, num_candidates=K, replicas=R, depth=D, root_envs=None,
                       root_players=p.data_ptr(), candidates=c.data_ptr(), seed=seed, terms=terms.data_ptr())
    rc = eng.L.gvec_search_playouts_bot(eng.h, C.byref(a), bot_players, permille)
    eng.synchronize()
    return rc, terms.cpu().numpy()


def _assert_terms_equal(got, want, ctx=""):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        i, k, j = bad[0]
        raise AssertionError(f"{ctx}: {len(bad)} of {got[..., 0].size} playouts differ; first root {i} candidate {k} replica {j}: "
                             f"kernel {got[i, k, j].tolist()} reference {want[i, k, j].tolist()} ({SR.TERMS})")


def _twins(mw, mh, maxp, sizes, fog=True, board_seed=3, prod=(1, 1, 1), interval=25):
    import generalsreinforcementlearning_amd as g
    boards = H.gen_boards(board_seed, sizes, mw, mh)
    eng = g.VecEngine(len(sizes), mw, mh, maxp, fog_of_war=fog, production=prod, normal_growth_interval=interval)
    ora = O.OracleBatch(len(sizes), mw, mh, maxp, fog=fog, prod=prod, interval=interval)
    eng.reset(*boards)
    ora.reset(*boards)
    return eng, ora


def _candidates(st, players, stride, fog, with_half=False):
    """[n, 3]: the seat's first legal move (with_half: its tile as a half move), its last legal move, the pass"""
    n = len(players)
    cand = np.full((n, 3), SR.NONE, np.int64)
    for i in range(n):
        legal = SR.legal_gym_actions(st, i, int(players[i]), stride, fog)
        if legal:
            cand[i, :2] = [legal[0] // 5 * 5 + 4 if with_half else legal[0], legal[-1]]
        cand[i, 2] = SR.PASS
    return cand


# ---- the roots whose playouts are won, lost and cut short -------------------------------------------------------------------
COVER_R, COVER_D = 2, 4


@pytest.mark.parametrize("bot_players,permille", [(0b11, 0), (0b10, 0), (0b11, 500)], ids=["both", "seat1", "both_mix500"])
@pytest.mark.parametrize("fog", [False, True], ids=["nofog", "fog"])
def test_coverage_roots_equal_the_reference(fog, bot_players, permille):
    import generalsreinforcementlearning_amd as g
    st, players, cand = SR.coverage_roots(fog)
    n = len(players)
    eng = g.VecEngine(n, SR.COVER_W, SR.COVER_H, SR.COVER_P, fog_of_war=fog)
    eng.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])
    eng.write_state({k: st[k] for k in SR.IMPORTED if k not in ("width", "height", "players")})   # those three came with the reset
    H.assert_states_equal(eng.game_state(), st, "the engine did not take the roots")
    want = SBR.reference_terms_bot(st, None, players, cand, COVER_R, COVER_D, SR.COVER_SEARCH_SEED, SR.COVER_W, SR.COVER_H, SR.COVER_P,
                                   bot_players, permille, fog=fog)
    valid = want[..., 0] == 1
    assert (want[..., 3] == 1).any() and (valid & (want[..., 2] == 0)).any() and (valid & (want[..., 1] < COVER_D)).any()
    got = _terms(eng, None, players, cand, COVER_R, COVER_D, SR.COVER_SEARCH_SEED, bot_players, permille)
    _assert_terms_equal(got, want, f"fog {fog} seats {bot_players:#b} permille {permille}")
    eng.close()


# ---- every compiled variant -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_every_variant_equals_the_reference(maxp, slots, parity):
    B, R, D, seed = 4, 2, 3, 11
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = _twins(mw, mh, maxp, sizes)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(B) + 1) % st["players"]                            # a seat that cycles over the env's players
    cand = _candidates(st, players, mw * mh, True)
    assert (cand[:, 0] >= 0).sum() >= B - 1
    every_seat = (1 << maxp) - 1
    want = SBR.reference_terms_bot(st, None, players, cand, R, D, seed, mw, mh, maxp, every_seat)
    assert (want[..., 0] == 1).sum() >= (B - 1) * 3 * R
    _assert_terms_equal(_terms(eng, None, players, cand, R, D, seed, every_seat), want, f"P{maxp} slots {slots} {parity}")
    eng.close()


# ---- wide armies and lists that differ from ownership -----------------------------------------------------------------------
def test_rare_state_forms_equal_the_reference():
    B, w, h, p, R, D, seed = 36, 10, 10, 4, 1, 3, 5
    eng, ora = _twins(w, h, p, [(w, h, p if i % 2 else 3) for i in range(B)], board_seed=21)
    H.run_lockstep(eng, ora, 20, seed=4, check_every=20, want_mask=False, ctx="youth")
    SF.age_batch(eng, 7)
    SF.age_batch(ora, 7)
    H.run_lockstep(eng, ora, 12, seed=13, invalid_permille=200, check_every=12, want_mask=False, ctx="ageing")
    st = eng.game_state()
    wide, desynced = SF.wide_envs(st), SF.desynced_envs(st)
    assert wide.sum() >= 4 and desynced.sum() >= 4 and (wide & desynced).any(), (wide.sum(), desynced.sum())
    fl = SF.check_flag_invariants(eng, st, "aged roots")
    assert (fl & SF.HF_WIDE).any() and (fl & SF.HF_LDIFF).any()
    players = np.arange(B) % st["players"]
    cand = _candidates(st, players, w * h, True, with_half=True)
    want = SBR.reference_terms_bot(st, None, players, cand, R, D, seed, w, h, p, 0b1111)
    live = want[..., 0] == 1
    assert live[wide].any() and live[desynced].any()
    _assert_terms_equal(_terms(eng, None, players, cand, R, D, seed, 0b1111), want, "aged roots")
    eng.close()


# ---- one shared engine for the tests below: 14x15 ragged boards, four players, 40 turns old -----------------------------------
SH_B, SH_R, SH_D, SH_SEED = 6, 2, 6, 23


def _shared_engine():
    mw, mh, sizes = H.variant_batch(4, 4, "odd", SH_B)
    eng, ora = _twins(mw, mh, 4, sizes)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(SH_B) + 1) % st["players"]
    return eng, ora, st, players, _candidates(st, players, mw * mh, True, with_half=True), (mw, mh)


def test_no_seat_on_the_rule_gives_the_existing_calls_terms():
    """bot_players == 0 runs the new kernel and must return what gvec_search_playouts returns, bit for bit - and so must a mix
    of 1000 per mille, where every seat on the rule plays the agent's draw every turn."""
    import generalsreinforcementlearning_amd as g
    eng, _, st, players, cand, _ = _shared_engine()
    s = g.PlayoutSearch(eng, candidates=cand.shape[1], replicas=SH_R, depth=SH_D)
    want = s.evaluate(None, _cuda(players, np.int32), _cuda(cand, np.int64), SH_SEED).cpu().numpy()
    assert (want[..., 0] == 1).sum() >= 3 * SH_R * (SH_B - 1) and (want[:, :, 0] != want[:, :, 1]).any()
    rc, got = _entry_point(eng, players, cand, SH_R, SH_D, SH_SEED, 0)
    assert rc == 0, eng.L.gvec_last_error()
    _assert_terms_equal(got, want, "no seat on the rule")
    rc, got = _entry_point(eng, players, cand, SH_R, SH_D, SH_SEED, 0b1111, 1000)
    assert rc == 0, eng.L.gvec_last_error()
    _assert_terms_equal(got, want, "every seat on the rule, always the agent's draw")
    # what needs a handle to be decided: a seat the handle does not have, and the no-op, which touches no pointer
    rc, got = _entry_point(eng, players, cand, SH_R, SH_D, SH_SEED, 0b10000)
    assert rc == -1 and b"gvec_search_playouts_bot: bot_players names a seat at or above max_players" in eng.L.gvec_last_error()
    assert (got == -7).all()
    rc, got = _entry_point(eng, players, cand, SH_R, SH_D, SH_SEED, 0b1111, 0, num_roots=0)
    assert rc == 0 and (got == -7).all()
    eng.close()


def _resident_bytes(eng):
    """everything the handle keeps per env, byte for byte: the canonical records of every env (header with the lifetime
    counters, planes, armies) and the raw header, legal-mask, action and err buffers"""
    import torch
    rec = torch.zeros(eng.B * eng.state_bytes_per_env(), dtype=torch.uint8, device="cuda")
    eng.export_records(rec.data_ptr())
    eng.synchronize()
    out = {"records": rec.cpu().numpy()}
    for name, which, per in (("header", 0, 24 * 4), ("legal", 3, eng.max_p * eng.mask_bytes), ("actions", 4, eng.max_p * 8), ("err", 5, 4)):
        buf = np.zeros(eng.B * per, np.uint8)
        assert eng.L.gvec_read_buffer(eng.h, which, 0, buf.size, buf.ctypes.data) == 0
        out[name] = buf
    return out


def test_the_roots_are_read_only():
    eng, ora, st, players, cand, _ = _shared_engine()
    twin, _, _, _, _, _ = _shared_engine()                                   # the same history, never searched
    eng.legal_action_mask_bits()                                             # the legal-mask buffer is current from here on
    before, counters = _resident_bytes(eng), eng.counters()
    got = _terms(eng, None, players, cand, SH_R, SH_D, SH_SEED, 0b1111, 100)
    assert (got[..., 0] == 1).any() and (got[..., 1] == SH_D).any()
    after = _resident_bytes(eng)
    for k in before:
        assert np.array_equal(before[k], after[k]), f"the search changed the handle's {k}"
    assert eng.counters() == counters
    H.assert_states_equal(eng.game_state(), st, "after the search")
    acts = ora.agent_actions(31)
    (e1, m1), (e2, m2) = eng.step(acts, want_mask=True), twin.step(acts, want_mask=True)
    assert np.array_equal(e1, e2) and np.array_equal(m1, m2)
    H.assert_states_equal(eng.game_state(), twin.game_state(), "the step after a search")
    assert eng.counters() == twin.counters()
    eng.close()
    twin.close()


@pytest.mark.parametrize("bot_players,permille", [(0b1111, 0), (0b0110, 300)], ids=["every_seat", "two_seats_mix300"])
def test_equals_the_composition_of_existing_calls_on_the_device(bot_players, permille):
    """copy_envs of every root K * R times into a scratch engine without a board pool; per turn agent_actions, bot_actions over
    them and one step, the seat's slot overridden on turn 0; the terms from game_state."""
    import generalsreinforcementlearning_amd as g
    eng, _, st, players, cand, (mw, mh) = _shared_engine()
    got = _terms(eng, None, players, cand, SH_R, SH_D, SH_SEED, bot_players, permille)
    plan = SR.Plan(st, None, players, cand, SH_R, mw, mh, 4, True)
    scratch = g.VecEngine(plan.V, mw, mh, 4)
    scratch.copy_envs(src_ids=plan.src.astype(np.int32), src=eng)
    turn0 = scratch.game_state(fields=("turn",))["turn"].astype(np.int64)
    assert np.array_equal(turn0, st["turn"][plan.src])
    moved = 0
    for t in range(SH_D):
        acts = scratch.agent_actions(SH_SEED)
        agent = acts.copy()
        scratch.bot_actions(bot_players, SH_SEED, permille, actions=acts)
        moved += int((acts != agent).any(axis=0).sum())
        scratch.step(plan.override(acts) if t == 0 else acts)
    assert moved > 0                                                        # the rule's moves are not the agent's
    _assert_terms_equal(got, plan.terms(turn0, scratch.game_state()), "device composition")
    assert (got[..., 0] == 1).sum() >= 3 * SH_R * (SH_B - 1)
    eng.close()
    scratch.close()


def test_the_same_call_gives_the_same_terms_and_replicas_differ():
    eng, _, st, players, cand, _ = _shared_engine()
    one = _terms(eng, None, players, cand, 4, SH_D, SH_SEED, 0b1111, 500)
    two = _terms(eng, None, players, cand, 4, SH_D, SH_SEED, 0b1111, 500)
    assert np.array_equal(one, two)
    valid = one[..., 0] == 1
    assert valid.sum() >= 3 * 4 * (SH_B - 1)
    assert (one[:, :, 0] != one[:, :, 1]).any(), "two replicas of one candidate never differ at 500 per mille"
    assert not np.array_equal(one, _terms(eng, None, players, cand, 4, SH_D, SH_SEED + 1, 0b1111, 500))
    eng.close()


# ---- the Python front -------------------------------------------------------------------------------------------------------
def test_act_returns_legal_actions():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(8, board_width=8, board_height=8, max_players=2, device_outputs=True, board_pool=16)
    search = g.PlayoutSearch(env, candidates=4, replicas=2, depth=4, rollout="bot")
    assert search.bot_players == 0b11
    obs, info = env.reset()
    for step in range(12):
        mask = info["valid_actions_mask"].view(-1, env.single_action_n)
        actions, found = search.act(mask, seed=step)
        has = mask.any(dim=1)
        assert bool(has.any())
        assert bool(mask.gather(1, actions[:, None]).squeeze(1)[has].all()), "act chose an action the mask refuses"
        assert bool(found["valid"].any(dim=1)[has].all())
        q = found["q"][found["valid"]]
        assert bool(torch.isfinite(q).all()) and float(q.abs().max()) <= 1.0
        obs, _, _, _, info = env.step(actions.view(env.num_envs, -1))
    env.close()


def test_an_arena_entrant_plays_its_games_to_the_end():
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(8, board_width=8, board_height=8, max_players=2, max_turns=40, device_outputs=True, board_pool=16)
    search = g.PlayoutSearch(env, candidates=4, replicas=2, depth=4, rollout="bot", bot_random_permille=100)
    policy = g.playout_policy(search, seed=1)
    arena = g.Arena(env, [policy, g.random_policy(seed=2)])
    steps = arena.run(episodes_per_env=1, poll_every=4, max_steps=200)
    res = arena.results()
    assert res.totals["games"] == 8 and set(res.totals["per_env"]["games"].tolist()) == {1}
    assert 1 <= steps <= 44 and policy._calls == steps
    env.close()
