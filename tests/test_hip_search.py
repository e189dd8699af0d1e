"""gvec_search_playouts on the GPU: its terms against the CPU reference (tests/_search_reference.py) exactly - every compiled
variant, the roots whose playouts end early, the rare state forms - that it reads its roots only, that it equals the
composition of existing calls on the device, its argument handling, and the Python front up to an Arena entrant."""
import re

import numpy as np
import pytest

import _harness as H
import _oracle as O
import _search_reference as SR
import _state_forms as SF

pytestmark = pytest.mark.gpu


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _terms(eng, env_ids, players, cand, R, D, seed):
    """the kernel's terms [n, K, R, 8] on the host"""
    import generalsreinforcementlearning_amd as g
    cand = np.asarray(cand, np.int64)
    s = g.PlayoutSearch(eng, candidates=cand.shape[1], replicas=R, depth=D)
    out = s.evaluate(None if env_ids is None else _cuda(env_ids, np.int32), _cuda(players, np.int32), _cuda(cand, np.int64), seed)
    return out.cpu().numpy()


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
    """[n, 5]: three accepted moves of the seat (first, middle, last of its list; with_half: the middle one's tile as a half
    move), the pass, padding"""
    n = len(players)
    cand = np.full((n, 5), SR.NONE, np.int64)
    for i in range(n):
        legal = SR.legal_gym_actions(st, i, int(players[i]), stride, fog)
        if legal:
            mid = legal[len(legal) // 2]
            cand[i, :3] = [legal[0], mid // 5 * 5 + 4 if with_half else mid, legal[-1]]
        cand[i, 3] = SR.PASS
    return cand


# ---- every compiled variant -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_every_variant_equals_the_reference(maxp, slots, parity):
    B, R, D, seed = 6, 2, 6, 11
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = _twins(mw, mh, maxp, sizes)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(B) + 1) % st["players"]                            # a seat that cycles over the env's players
    cand = _candidates(st, players, mw * mh, True)
    assert (cand[:, 0] >= 0).sum() >= B - 1
    want = SR.reference_terms(st, None, players, cand, R, D, seed, mw, mh, maxp)
    assert (want[:, :4, :, 0] == 1).sum() >= (B - 1) * 4 * R and not want[:, 4].any()
    _assert_terms_equal(_terms(eng, None, players, cand, R, D, seed), want, f"P{maxp} slots {slots} {parity}")
    eng.close()


# ---- the roots whose playouts are won, lost and cut short -------------------------------------------------------------------
@pytest.mark.parametrize("mix", [(6554, 19661), (0, 0)], ids=["default_mix", "always_move"])
@pytest.mark.parametrize("fog", [False, True], ids=["nofog", "fog"])
def test_coverage_roots_equal_the_reference(fog, mix):
    import generalsreinforcementlearning_amd as g
    st, players, cand = SR.coverage_roots(fog)
    n = len(players)
    eng = g.VecEngine(n, SR.COVER_W, SR.COVER_H, SR.COVER_P, fog_of_war=fog)
    eng.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])
    eng.write_state({k: st[k] for k in SR.IMPORTED if k not in ("width", "height", "players")})   # those three came with the reset
    H.assert_states_equal(eng.game_state(), st, "the engine did not take the roots")
    eng.set_agent_mix(*mix)
    want = SR.reference_terms(st, None, players, cand, SR.COVER_R, SR.COVER_D, SR.COVER_SEARCH_SEED, SR.COVER_W, SR.COVER_H, SR.COVER_P,
                              fog=fog, mix=mix)
    valid = want[..., 0] == 1
    assert (want[..., 3] == 1).any() and (valid & (want[..., 2] == 0)).any() and (valid & (want[..., 1] < SR.COVER_D)).any()
    _assert_terms_equal(_terms(eng, None, players, cand, SR.COVER_R, SR.COVER_D, SR.COVER_SEARCH_SEED), want, f"fog {fog} mix {mix}")
    eng.close()


# ---- wide armies and lists that differ from ownership -----------------------------------------------------------------------
def test_rare_state_forms_equal_the_reference():
    B, w, h, p, R, D, seed = 36, 10, 10, 4, 2, 6, 5
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
    want = SR.reference_terms(st, None, players, cand, R, D, seed, w, h, p)
    live = want[..., 0] == 1
    assert live[wide].any() and live[desynced].any()
    _assert_terms_equal(_terms(eng, None, players, cand, R, D, seed), want, "aged roots")
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
    got = _terms(eng, None, players, cand, SH_R, SH_D, SH_SEED)
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


def test_equals_the_composition_of_existing_calls_on_the_device():
    """copy_envs of every root K * R times into a scratch engine without a board pool, one step with the agent's moves and the
    seat's slot overridden, a fused rollout of depth - 1, the terms from game_state."""
    import generalsreinforcementlearning_amd as g
    eng, _, st, players, cand, (mw, mh) = _shared_engine()
    got = _terms(eng, None, players, cand, SH_R, SH_D, SH_SEED)
    plan = SR.Plan(st, None, players, cand, SH_R, mw, mh, 4, True)
    scratch = g.VecEngine(plan.V, mw, mh, 4)
    scratch.copy_envs(src_ids=plan.src.astype(np.int32), src=eng)
    turn0 = scratch.game_state(fields=("turn",))["turn"].astype(np.int64)
    assert np.array_equal(turn0, st["turn"][plan.src])
    scratch.step(plan.override(scratch.agent_actions(SH_SEED)))
    scratch.rollout(SH_D - 1, SH_SEED, fused=True)
    _assert_terms_equal(got, plan.terms(turn0, scratch.game_state()), "device composition")
    assert (got[..., 0] == 1).sum() >= 4 * SH_R * (SH_B - 1)
    eng.close()
    scratch.close()


def test_arguments_on_the_device():
    import torch
    import generalsreinforcementlearning_amd as g
    eng, _, st, players, cand, (mw, mh) = _shared_engine()
    want = SR.reference_terms(st, None, players, cand, SH_R, SH_D, SH_SEED, mw, mh, 4)
    # root ids: a permutation with repeats, and ids outside the batch -> zero rows, the others as they must be
    ids = np.array([3, 3, SH_B, 0, -1, 5, 2 ** 30, 1], np.int32)
    seats, picked = players[np.clip(ids, 0, SH_B - 1)], cand[np.clip(ids, 0, SH_B - 1)]
    eng.legal_action_mask_bits()
    before = _resident_bytes(eng)
    got = _terms(eng, ids, seats, picked, SH_R, SH_D, SH_SEED)
    ref = SR.reference_terms(st, ids, seats, picked, SH_R, SH_D, SH_SEED, mw, mh, 4)
    _assert_terms_equal(got, ref, "explicit root ids")
    outside = (ids < 0) | (ids >= SH_B)
    assert not got[outside].any() and (got[~outside][..., 0] == 1).any()
    after = _resident_bytes(eng)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # NULL root_envs is arange
    _assert_terms_equal(_terms(eng, None, players, cand, SH_R, SH_D, SH_SEED), want, "NULL root ids")
    _assert_terms_equal(_terms(eng, np.arange(SH_B), players, cand, SH_R, SH_D, SH_SEED), want, "arange root ids")
    # a seat outside the env, and one outside the handle
    odd = players.copy()
    odd[0], odd[1], odd[2] = 7, -1, st["players"][2]
    got = _terms(eng, None, odd, cand, SH_R, SH_D, SH_SEED)
    _assert_terms_equal(got, SR.reference_terms(st, None, odd, cand, SH_R, SH_D, SH_SEED, mw, mh, 4), "odd seats")
    assert not got[0].any() and not got[1].any()
    # n = 0 is a no-op: through the front and through the entry point, whose pointers it must not touch
    s = g.PlayoutSearch(eng, candidates=5, replicas=SH_R, depth=SH_D)
    empty = s.evaluate(None, torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros((0, 5), dtype=torch.int64, device="cuda"))
    assert tuple(empty.shape) == (0, 5, SH_R, 8)
    eng.search_playouts_device(0, 16, 16, 16, 5, SH_R, SH_D)
    # the entry point names what it refuses (a real handle: refused before any launch)
    for kw, text in ((dict(num_candidates=0), "num_candidates"), (dict(replicas=-1), "replicas"), (dict(depth=0), "depth"),
                     (dict(num_roots=-2), "num_roots"), (dict(terms_ptr=None), "terms"), (dict(num_roots=2 ** 30, num_candidates=4), "2^31")):
        a = dict(num_roots=1, candidates_ptr=16, root_players_ptr=16, terms_ptr=16, num_candidates=5, replicas=2, depth=3)
        a.update(kw)
        with pytest.raises(g.GvecError, match=re.escape(text)):
            eng.search_playouts_device(**a)
    # the front refuses what the kernel cannot read
    c, p = _cuda(cand, np.int64), _cuda(players, np.int32)
    wide = torch.zeros((SH_B, 10), dtype=torch.int64, device="cuda")
    for bad in (lambda: s.evaluate(None, p, wide[:, ::2]), lambda: s.evaluate(None, p.cpu(), c), lambda: s.evaluate(None, p, c.cpu()),
                lambda: s.evaluate(torch.arange(SH_B), p, c), lambda: s.evaluate(None, p.to(torch.int64), c),
                lambda: s.evaluate(None, p[:-1], c), lambda: s.evaluate(None, p, c[:, :4])):
        with pytest.raises(ValueError):
            bad()
    eng.synchronize()
    eng.close()


# ---- the Python front -------------------------------------------------------------------------------------------------------
def test_act_finds_the_capture_of_the_enemy_general():
    """5x5, two players: seat 0 holds 50 armies on (3, 4), next to seat 1's general on (4, 4).  Of seat 0's seven legal actions
    and the pass exactly one - (3, 4) moving right - takes the general, which ends the game on the playout's first turn.
    The agent mix is "never move": a move of seat 1 from the general just taken would abort that turn (ErrNotOwned), and an
    aborted turn skips the game-over check until the next one."""
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    W = H_ = 5
    env = GeneralsSelfPlayVecEnv(2, board_width=W, board_height=H_, max_players=2, device_outputs=True, board_pool=4)
    env.reset()
    tiles = [dict(x=0, y=0, owner=0, army=5, type=1), dict(x=4, y=4, owner=1, army=2, type=1), dict(x=3, y=4, owner=0, army=50)]
    army, owner, typ = O.planes_from_tiles(W, H_, tiles)
    env.engine.reset(np.stack([army] * 2), np.stack([owner] * 2), np.stack([typ] * 2))
    env.engine.set_agent_mix(65536, 0)
    st = env.engine.game_state()
    capture = (4 * W + 3) * 5 + 1
    mask = np.zeros((4, W * H_ * 5), bool)                                   # rows (env, column): seat = row % 2
    for r in range(4):
        for a in range(W * H_ * 5):
            mask[r, a] = SR.decode_candidate(st, r // 2, r % 2, a, W * H_, True) is not None or \
                (a % 5 == 4 and any(SR.decode_candidate(st, r // 2, r % 2, a - 4 + d, W * H_, True) is not None for d in range(4)))
    assert mask[0].sum() == 7 and mask[0, capture]
    search = g.PlayoutSearch(env, candidates=8, replicas=4, depth=5)
    actions, info = search.act(torch.from_numpy(mask).cuda(), seed=3)
    cand, terms, valid, q = (info[k].cpu().numpy() for k in ("candidates", "terms", "valid", "q"))
    assert actions.cpu().tolist()[0::2] == [capture, capture]
    for r in (0, 2):
        k = int(np.flatnonzero(cand[r] == capture)[0])
        assert terms[r, k, :, 3].tolist() == [1] * 4 and terms[r, k, :, 1].tolist() == [1] * 4 and terms[r, k, :, 0].tolist() == [1] * 4
        others = [j for j in range(8) if j != k]
        assert not terms[r, others][..., 3].any()
        assert valid[r].sum() == 7 and sorted(cand[r][valid[r]].tolist()) == np.flatnonzero(mask[0]).tolist()
        assert q[r, k] == 1.0 and (q[r, others] < 1.0).all()
    # the pass and the moves beside the capture, straight through evaluate: nobody wins on the first turn
    c = np.array([[capture, SR.PASS, capture - 1, 0 * 5 + 1]], np.int64)
    t = _terms(env.engine, [0], [0], c, 4, 1, 9)
    assert t[0, :, :, 0].all() and t[0, 0, :, 3].all() and not t[0, 1:, :, 3].any() and (t[0, :, :, 1] == 1).all()
    # the policy target: a distribution over the valid candidates, or nothing
    target = search.policy_target(info["candidates"], info["q"], info["valid"], temperature=0.5)
    assert tuple(target.shape) == (4, W * H_ * 5) and target.dtype == torch.float32
    sums = target.double().sum(dim=1).cpu().numpy()
    has = valid.any(axis=1)
    assert has.all() and np.abs(sums - 1.0).max() < 1e-6
    assert ((target > 0).cpu().numpy() <= mask).all() and int(target[0].argmax()) == capture
    none = search.policy_target(info["candidates"], info["q"], torch.zeros_like(info["valid"]))
    assert float(none.abs().sum()) == 0.0
    env.close()


def test_an_arena_entrant_plays_legal_actions():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(16, board_width=8, board_height=8, max_players=2, device_outputs=True, board_pool=32)
    search = g.PlayoutSearch(env, candidates=4, replicas=2, depth=4)
    policy = g.playout_policy(search, seed=1)
    arena = g.Arena(env, [policy, g.random_policy(seed=2)])
    assert policy._rows is arena._rows[0] and int(policy._rows.numel()) == 16
    seats = search._rows_to_ids(16, policy._rows)
    assert torch.equal(seats[0].cpu(), (policy._rows // 2).to(torch.int32).cpu())
    assert seats[1].cpu().tolist() == [int(r) % 2 for r in policy._rows.cpu().tolist()]
    invalid = torch.zeros((16, 2), dtype=torch.int32, device="cuda")
    for _ in range(20):
        out = arena.step()
        invalid += out[4]["invalid"].to(torch.int32)
    assert int(invalid.sum()) == 0
    assert policy._calls == 20
    env.close()
