"""Configurable rewards on the device: gvec_experience_rewards_config and the reward-only snapshot against the numpy restatement
of CalculateRewardWithConfig (tests/_reward_reference.py) on the oracle twin's states - float32, tolerance 0 - and the gym
vector envs' reward_config option against the same calls made by hand."""
import importlib.util
import math
import os

import numpy as np
import pytest

import _harness as H
import _oracle as O
import _reward_cases as RC
import _reward_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("owner", "army", "type", "alive", "players", "width", "height", "turn")


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


_bits = RC.bits


# the scripted bot plays `bots`; the other seats are the random agent.  On the CPU oracle (tests/_bot_reference.py playing the
# same seats) these rollouts hold every event the assertions at the end ask for.
@pytest.mark.parametrize("name,w,h,P,bots", [("10x10_p2", 10, 10, 2, 1), ("20x20_p4", 20, 20, 4, 3), ("21x13_p3", 21, 13, 3, 1)])
def test_configured_rewards_and_terms_equal_the_restatement(g, name, w, h, P, bots):
    B, turns, seed = 64, 250, 7
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, [(w, h, P)] * B, w, h)
    full = g.VecEngine(B, w, h, P, auto_reset=True)          # takes the full snapshot, answers the old entry point too
    lean = g.VecEngine(B, w, h, P, auto_reset=True)          # takes the reward-only snapshot
    ora = O.OracleBatch(B, w, h, P)
    for e in (full, lean, ora):
        e.reset(army, owner, typ, ws, hs, ps)
    full.build_board_pool(17, 4)
    lean.build_board_pool(17, 4)
    ora.set_pool(17, 4)
    cfgs = RC.configs(g.RewardConfig)
    rng = np.random.default_rng(seed)
    seen = np.zeros(8, np.int64)
    wins = redeals = clipped = penalised = 0
    subset = [P - 1] if P == 2 else [0, P - 1]
    for k in range(turns):
        acts = ora.agent_actions(seed + 5)
        full.bot_actions(bots, actions=acts)
        prev = ora.read_state(fields=STATE)
        full.experience_begin()
        lean.experience_begin(rewards_only=True)
        err = ora.step(acts)
        assert np.array_equal(full.step(acts), err) and np.array_equal(lean.step(acts), err)
        cur = ora.read_state(fields=STATE)
        live = R.comparable_rows(prev, cur)
        # the old entry point, the new one after the full snapshot, the new one after the reward-only snapshot: the same bytes
        r_old, d_old = full.experience_rewards()
        r_full, d_full, t_full = full.experience_rewards(config=cfgs["go_default"], terms=True)
        r_lean, d_lean, t_lean = lean.experience_rewards(config=cfgs["go_default"], terms=True)
        assert r_old.tobytes() == r_full.tobytes() == r_lean.tobytes(), (name, k)
        assert np.array_equal(d_old, d_full) and np.array_equal(d_old, d_lean) and t_full.tobytes() == t_lean.tobytes()
        for cname, cfg in cfgs.items():
            inv = (rng.random((B, P)) < 0.1) if cname == "clip" else None
            r, d, t = lean.experience_rewards(config=cfg, invalid=inv, terms=True)
            wr, wt, wd = R.reward_reference(prev, cur, cfg, invalid=inv)
            assert np.array_equal(_bits(r), _bits(wr)), (name, cname, k, r[r != wr][:4], wr[r != wr][:4])
            assert np.array_equal(t, wt), (name, cname, k)
            assert np.array_equal(d, wd)
            # rewards = the terms recombined in the definition's order, then the three rules
            raw = R.recombine(t, cfg)
            want = R.normalize_reward(raw) if cfg.clip else raw
            want = np.where(live[:, None] & (np.arange(P)[None] < cur["players"][:, None]), want, np.float32(0))
            if inv is not None:
                want = np.where(inv, want + np.float32(cfg.invalid_action), want)
                penalised += int((inv & ~live[:, None]).sum())
            assert np.array_equal(_bits(r), _bits(want.astype(np.float32))), (name, cname, k)
            if cname == "clip":
                hit = (np.abs(raw) > 1) & live[:, None]
                clipped += int(hit.sum())
                assert np.all(np.abs(r[hit & ~inv]) == 1.0)
        if k % 10 == 0:       # a players subset: the matching columns, terms and all
            rs, ds, ts = lean.experience_rewards(config=cfgs["awkward"], players=subset, terms=True)
            ra, _, ta = lean.experience_rewards(config=cfgs["awkward"], terms=True)
            assert rs.tobytes() == np.ascontiguousarray(ra[:, subset]).tobytes() and ts.tobytes() == np.ascontiguousarray(ta[:, subset]).tobytes()
        seen += (t_lean != 0).sum((0, 1))
        wins += int((t_lean[..., 6] > 0).sum())
        redeals += int((~live).sum())
    H.assert_states_equal(lean.game_state(), ora.read_state(), name)
    assert seen[2] >= 1 and seen[3] >= 1, f"{name}: cities gained / lost {seen[2]} / {seen[3]}"
    assert seen[4] >= 1 and seen[5] >= 1, f"{name}: generals captured / lost {seen[4]} / {seen[5]}"
    assert wins >= 1 and redeals >= 1 and clipped >= 1 and penalised >= 1, (name, wins, redeals, clipped, penalised)


def test_entry_point_refusals_that_need_a_handle(g):
    import ctypes as C
    eng = g.VecEngine(4, 8, 8, 3)
    eng.reset_generated(3)
    cfg = g.RewardConfig.go_default().to_c()
    out = np.zeros((4, 3), np.float32)
    L = eng.L
    assert L.gvec_experience_rewards_config(eng.h, C.byref(cfg), 1 << 3, None, out.ctypes.data, None, None, 0) == -1
    assert b"at or above max_players = 3" in L.gvec_last_error()
    assert L.gvec_experience_rewards_config(eng.h, C.byref(cfg), 0, None, out.ctypes.data, None, None, 0) == -1
    assert b"without a preceding" in L.gvec_last_error()
    eng.experience_begin(rewards_only=True)
    r, d = eng.experience_rewards(config=g.RewardConfig.go_default())
    assert r.shape == (4, 3) and not r.any() and not d.any()         # nothing was stepped: no predecessor, reward 0
    done_only = np.ones(4, np.uint8)
    assert L.gvec_experience_rewards_config(eng.h, C.byref(cfg), 0, None, None, None, done_only.ctypes.data, 0) == 0 and not done_only.any()


def test_sharded_handle_gives_the_single_device_answers(g):
    """three shards on one device against a plain handle: the reward-only snapshot and the configured rewards fan out with the
    caller's host arrays offset per shard (invalid, rewards, terms, done)"""
    B, w, h, P = 50, 10, 10, 3
    one = g.VecEngine(B, w, h, P, auto_reset=True)
    many = g.VecEngine(B, w, h, P, auto_reset=True, devices=[0, 0, 0])
    cfg = RC.configs(g.RewardConfig)["clip"]
    rng = np.random.default_rng(4)
    for e in (one, many):
        e.reset_generated(5)
        e.build_board_pool(6, 1)
        e.rollout(40, 3, 5, fused=True, want_stats=False)
    for k in range(6):
        acts = one.agent_actions(11 + k, 6)
        inv = rng.random((B, 2)) < 0.3
        for e in (one, many):
            e.experience_begin(rewards_only=True)
            e.step(acts)
        a, b = (e.experience_rewards(config=cfg, players=[0, 2], invalid=inv, terms=True) for e in (one, many))
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes(), k
        assert a[0].any() and a[2].any()
    one.close()
    many.close()


# ---- the gym vector envs -----------------------------------------------------------------------------------------------------

def _actions(torch, mask, step, bad_share):
    """a valid action per learner where there is one (drawn from the mask), and an index the mask refuses for a share of them"""
    gen = torch.Generator(device=mask.device)
    gen.manual_seed(1000 + step)
    score = mask.float() * torch.rand(mask.shape, device=mask.device, generator=gen)
    good = score.argmax(-1)
    bad = (~mask).float().mul(torch.rand(mask.shape, device=mask.device, generator=gen)).argmax(-1)
    pick_bad = torch.rand(good.shape, device=mask.device, generator=gen) < bad_share
    return torch.where(pick_bad, bad, good)


def _run_env_triplet(g, make, learners_of, B=48, w=9, h=7, steps=40):
    """make(B, w, h, **options) -> an env.  on: reward_config; off: the same env without it; hand: without it, the three
    launches made by hand around its step"""
    import torch
    cfg = g.RewardConfig(capture_city=3.0, lose_city=-3.0, territory_gained=0.25, territory_lost=-0.25, invalid_action=-0.375, clip=True)
    on, off, hand = make(B, w, h, reward_config=cfg), make(B, w, h), make(B, w, h)
    o_on, i_on = on.reset(seed=5)
    o_off, i_off = off.reset(seed=5)
    hand.reset(seed=5)
    assert torch.equal(o_on, o_off) and torch.equal(i_on["valid_actions_mask"], i_off["valid_actions_mask"])
    flags = [name for name, _ in on._INFO_FLAGS] + ["turn", "winner", "reset", "valid_actions_mask"]
    refused = redealt = nonzero = 0
    for k in range(steps):
        a = _actions(torch, i_off["valid_actions_mask"], k, 0.15)
        o_on, r_on, te_on, tr_on, i_on = on.step(a)
        o_off, r_off, te_off, tr_off, i_off = off.step(a)
        hand.engine.experience_begin()
        _, _, te_h, _, i_h = hand.step(a)
        inv = i_h["invalid_action" if "invalid_action" in i_h else "invalid"]
        want, _, terms = hand.engine.experience_rewards(config=cfg, players=learners_of(hand), invalid=inv.cpu().numpy(), terms=True)
        assert torch.equal(o_on, o_off) and torch.equal(te_on, te_off) and torch.equal(tr_on, tr_off), k
        for f in flags:
            assert torch.equal(i_on[f], i_off[f]), (k, f)
        assert set(i_on) == set(i_off) | {"reward_terms"}
        assert r_on.dtype == torch.float64 and r_on.shape == r_off.shape
        got = r_on.cpu().numpy()
        assert np.array_equal(got, want.astype(np.float64).reshape(got.shape)), (k, got[got != want.reshape(got.shape)][:4])
        assert np.array_equal(i_on["reward_terms"].cpu().numpy(), terms.reshape(tuple(got.shape) + (8,)))
        refused += int(inv.sum())
        redealt += int(i_on["reset"].sum())
        nonzero += int((got != 0).sum())
        if bool(i_on["reset"].any()):                   # a re-dealt row has no predecessor: 0, or exactly invalid_action
            rows = got[i_on["reset"].cpu().numpy()]
            assert np.isin(rows, [0.0, -0.375]).all()
    assert refused >= 1 and redealt >= 1 and nonzero >= 1, (refused, redealt, nonzero)
    for e in (on, off, hand):
        e.close()


@pytest.mark.parametrize("opponent", ["random", "bot"])
def test_single_learner_env_with_reward_config(g, opponent):
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    make = lambda B, w, h, **kw: GeneralsVecEnv(B, w, h, 2, max_turns=12, seed=5, board_pool=32, device_outputs=True,   # noqa: E731
                                                opponent=opponent, **kw)
    _run_env_triplet(g, make, lambda env: [env.player_id])


def test_single_learner_env_refused_action_is_exactly_invalid_action(g):
    """this env does not play a refused turn, so that row has no predecessor: 0 + invalid_action"""
    import torch
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    cfg = g.RewardConfig.clipped(invalid_action=-0.625)
    env = GeneralsVecEnv(16, 8, 8, 2, seed=3, board_pool=8, device_outputs=True, reward_config=cfg)
    _, info = env.reset()
    bad = (~info["valid_actions_mask"]).float().argmax(-1)
    _, r, _, _, info = env.step(bad)
    assert bool(info["invalid_action"].all()) and torch.equal(r, torch.full_like(r, -0.625)) and not bool(info["reward_terms"].any())
    env.close()


@pytest.mark.parametrize("players,learners", [(2, None), (3, [0, 2]), (8, None), (8, [1, 4, 7])])
def test_selfplay_env_with_reward_config(g, players, learners):
    """eight seats on 16x16 (the map generator needs 240 tiles to seat eight): with every seat a learner reward_terms is
    [B, 8, 8], one dword per lane of the kernel's wavefront"""
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    make = lambda B, w, h, **kw: GeneralsSelfPlayVecEnv(B, w, h, players, learners=learners, max_turns=12, seed=5,   # noqa: E731
                                                        board_pool=32, device_outputs=True, **kw)
    _run_env_triplet(g, make, lambda env: env.player_ids, **(dict(B=24, w=16, h=16) if players == 8 else {}))


def test_numpy_mode_returns_the_same_rewards(g):
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    cfg = g.RewardConfig.clipped()
    dev = GeneralsSelfPlayVecEnv(16, 8, 8, 2, seed=9, board_pool=8, device_outputs=True, reward_config=cfg)
    host = GeneralsSelfPlayVecEnv(16, 8, 8, 2, seed=9, board_pool=8, reward_config=cfg)
    _, i_d = dev.reset()
    host.reset()
    for k in range(6):
        import torch
        a = _actions(torch, i_d["valid_actions_mask"], k, 0.2)
        _, r_d, _, _, i_d = dev.step(a)
        _, r_h, _, _, i_h = host.step(a.cpu().numpy())
        assert r_h.dtype == np.float64 and np.array_equal(r_h, r_d.cpu().numpy()) and "reward_terms" not in i_h
    dev.close()
    host.close()


def test_rollout_buffer_stores_the_configured_rewards(g):
    """SelfPlayRolloutBuffer stores what step returns: 8 steps on an env with a clipped config end with finite returns inside the
    config's scale (every reward lies in [-1 - 0.1, 1]; with zero values and a zero bootstrap a return is a discounted sum of at most 8
    of them)."""
    import torch
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    cfg = g.RewardConfig.clipped()
    env = GeneralsSelfPlayVecEnv(32, 8, 8, 2, max_turns=6, seed=2, board_pool=16, device_outputs=True, reward_config=cfg)
    buf = g.SelfPlayRolloutBuffer(env, horizon=8, gamma=0.99, gae_lambda=0.95)
    buf.begin(*env.reset())
    zeros = torch.zeros((32, 2), device="cuda")
    bound = float(np.float32(1.0) + np.float32(0.1))       # |clip| + |invalid_action| as float32 adds them
    for k in range(8):
        a = _actions(torch, buf.valid_actions_mask, k, 0.2)
        _, r, _, _, info = buf.step(a, zeros, zeros)
        assert torch.equal(buf.reward[k].view(32, 2), r)
        assert float(r.abs().max()) <= bound
    buf.finish(zeros)
    ret = buf.returns
    assert bool(torch.isfinite(ret).all()) and float(ret.abs().max()) <= 8 * bound
    assert float(buf.reward.abs().sum()) > 0
    env.close()


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_ppo_example_runs_with_the_go_reward():
    out = _example("train_ppo_selfplay").main(["--reward", "go", "--num-envs", "64", "--board", "8", "--players", "2", "--horizon", "8",
                                               "--iterations", "2", "--batch-size", "512", "--max-turns", "10"])
    assert out["reward"] == "go" and len(out["iterations"]) == 2
    for r in out["iterations"]:
        assert all(math.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "clip_fraction")), r
    assert out["bad_actions"] == 0 and out["rejected"] == 0


def test_c51_example_sizes_its_support_from_the_config():
    out = _example("train_dqn_resident").main(["--reward", "sparse", "--categorical", "--num-envs", "128", "--board", "8", "--buffer-size",
                                               "20000", "--batch-size", "128", "--updates", "4", "--warmup-steps", "4",
                                               "--max-steps-per-episode", "20"])
    assert out["reward"] == "sparse" and (out["v_min"], out["v_max"]) == (-1.1, 1.1)
    assert out["updates"] == 4 and all(math.isfinite(x) for x in out["loss"])
