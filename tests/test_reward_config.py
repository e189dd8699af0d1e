"""Configurable rewards without a device: the numpy restatement of CalculateRewardWithConfig (tests/_reward_reference.py) against
the oracle and the reference's own test vectors, RewardConfig's refusals, and the C-side argument checks of
gvec_experience_rewards_config (which come before the handle or a device is looked at)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _harness as H
import _oracle as O
import _reward_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reward_config_kats.json")) as f:
    KATS = json.load(f)["cases"]

STATE = ("owner", "army", "type", "alive", "players", "width", "height", "turn")


def _cfg(**kw):
    from generalsreinforcementlearning_amd import RewardConfig
    return RewardConfig(**kw)


@pytest.mark.parametrize("name,B,size,turns,seed", [("6x6_p2", 48, (6, 6, 2), 300, 3), ("9x7_p3", 48, (9, 7, 3), 300, 11)])
def test_restatement_equals_the_oracle_bit_for_bit(name, B, size, turns, seed):
    """go_default() == ora_calculate_reward for every player of every env over rollouts with re-deals: tolerance 0.  The rollouts
    must contain what the terms are about - asserted from the restatement's own terms."""
    w, h, P = size
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, [size] * B, w, h)
    ora = O.OracleBatch(B, w, h, P)
    ora.reset(army, owner, typ, ws, hs, ps)
    ora.set_pool(17, 4)
    cfg = _cfg()
    seen = np.zeros(8, np.int64)
    wins = redeals = 0
    for k in range(turns):
        acts = ora.agent_actions(seed + 5)
        prev = ora.read_state(fields=STATE)
        ora.experience_begin()
        ora.step(acts)
        cur = ora.read_state(fields=STATE)
        orr, od = ora.rewards()
        r, t, done = R.reward_reference(prev, cur, cfg)
        assert np.array_equal(r.view(np.uint32), orr.view(np.uint32)), (name, k, r[r != orr][:4], orr[r != orr][:4])
        assert np.array_equal(done, od.astype(bool))
        assert np.array_equal(R.recombine(t, cfg).view(np.uint32)[R.comparable_rows(prev, cur)], r.view(np.uint32)[R.comparable_rows(prev, cur)])
        seen += (t != 0).sum((0, 1))
        wins += int((t[..., 6] > 0).sum())
        redeals += int((~R.comparable_rows(prev, cur)).sum())
    assert seen[2] > 0 and seen[3] > 0, f"{name}: no city changed hands both ways: {seen}"
    assert seen[4] > 0 and seen[5] > 0, f"{name}: no general was captured: {seen}"
    assert wins > 0 and redeals > 0, (name, wins, redeals)


def _state(c, tiles, turn, alive=None):
    w, h, P = c["w"], c["h"], c["players"]
    army, owner, typ = O.planes_from_tiles(w, h, tiles)
    return {"army": army[None], "owner": owner[None], "type": typ[None], "alive": np.asarray([alive or [1] * P], np.uint8),
            "players": np.array([P], np.int32), "width": np.array([w], np.int32), "height": np.array([h], np.int32),
            "turn": np.array([turn], np.int32)}


@pytest.mark.parametrize("c", [pytest.param(c, id=c["name"]) for c in KATS])
def test_reference_test_vectors(c):
    """rewards_test.go:17-118 as data: exact where Go asserts Equal, within Go's own delta where it asserts InDelta."""
    cfg = _cfg()
    prev, cur = _state(c, c["prev"], 1), _state(c, c["cur"], 2, c["alive_cur"])
    r, t, done = R.reward_reference(prev, cur, cfg, players=[c["player"]])
    e = c["expect"]
    # Go's expected expression, in float32 as Go evaluates it
    want = np.float32(0)
    for field, mult in e["terms"]:
        want = want + np.float32(mult) * np.float32(getattr(cfg, field))
    a = e["advantage"]
    if a is not None:
        adv = lambda mine, other: np.float32(mine - other) / np.float32(mine + other)    # noqa: E731
        part = adv(a["player_armies"], a["enemy_armies"]) if a["kind"] == "current" else adv(*a["cur"]) - adv(*a["prev"])
        want = want + np.float32(part) * np.float32(cfg.army_advantage)
    assert abs(float(want) - e["value"]) < 1e-6                     # the fixture's evaluated value says the same
    assert not done[0]
    if e["match"] == "equal":
        assert r[0, 0] == want, (r, want)
    else:
        assert abs(float(r[0, 0]) - float(want)) <= e["delta"], (r, want)


def test_clip_zero_and_invalid_action_rules():
    """The three rules on top of the Go function, on the general-capture vector: NormalizeReward, the zero of a row that was not
    stepped, invalid_action after both."""
    c = next(k for k in KATS if k["name"].endswith("general_capture"))
    big = _cfg(capture_general=7.0, lose_general=-7.0, invalid_action=-0.25, clip=True)
    prev, cur = _state(c, c["prev"], 1), _state(c, c["cur"], 2, c["alive_cur"])
    r, t, _ = R.reward_reference(prev, cur, big, invalid=np.array([[0, 1]]))
    assert r[0, 0] == np.float32(1.0) and r[0, 1] == np.float32(-1.0) + np.float32(-0.25)
    assert t[0, 0, 4] == 1 and t[0, 1, 5] == 1 and t[0, 0, 6] == 0
    same_turn = _state(c, c["cur"], 1, c["alive_cur"])
    r, t, _ = R.reward_reference(prev, same_turn, big, invalid=np.array([[1, 0]]))
    assert r[0, 0] == np.float32(-0.25) and r[0, 1] == 0 and not t.any()
    # a finished game: the outcome replaces the shaped terms (rewards.go:49-56)
    r, t, done = R.reward_reference(prev, _state(c, c["cur"], 2, [1, 0]), _cfg(win_game=3.0, lose_game=-2.0))
    assert done[0] and list(r[0]) == [3.0, -2.0] and list(t[0, :, 6]) == [1, -1]


def test_reward_config_refusals_and_presets():
    from generalsreinforcementlearning_amd import REWARD_TERMS, RewardConfig
    d = RewardConfig.go_default()
    assert (d.win_game, d.lose_game, d.capture_city, d.lose_city, d.capture_general, d.lose_general, d.territory_gained, d.territory_lost,
            d.army_gained, d.army_lost, d.army_advantage, d.invalid_action, d.clip) == (1.0, -1.0, 0.1, -0.1, 0.5, -0.5, 0.01, -0.01, 0.001,
                                                                                         -0.001, 0.05, 0.0, False)     # rewards.go:23-37
    assert REWARD_TERMS == R.TERMS
    with pytest.raises(ValueError, match="never reads territory_lost"):
        RewardConfig(territory_lost=-0.5)
    with pytest.raises(ValueError, match="never reads army_lost"):
        RewardConfig(army_gained=0.002)
    RewardConfig(territory_gained=0.3, territory_lost=-0.3, army_gained=-0.7, army_lost=0.7)
    for bad in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="finite number"):
            RewardConfig(win_game=bad)
    with pytest.raises(ValueError, match="clip"):
        RewardConfig(clip=1)
    s = RewardConfig.sparse()
    assert (s.win_game, s.lose_game) == (1.0, -1.0) and not any((s.capture_city, s.lose_city, s.capture_general, s.lose_general,
                                                                  s.territory_gained, s.army_gained, s.army_advantage, s.invalid_action))
    assert RewardConfig.clipped().clip and RewardConfig.clipped().scale() == pytest.approx(1.1) and RewardConfig(win_game=5.0).scale() == 5.0
    c = RewardConfig(territory_gained=0.25, territory_lost=-0.25, invalid_action=-0.5, clip=True).to_c()
    assert (c.territory, c.invalid_action, c.flags, c.reserved) == (0.25, -0.5, 1, 0)


def test_c_default_config_is_the_references():
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import RewardConfigC
    L = g.load()
    c = RewardConfigC(reserved=7, flags=3, invalid_action=9.0)
    assert L.gvec_reward_config_default(C.byref(c)) == 0
    want = g.RewardConfig.go_default().to_c()
    assert bytes(c) == bytes(want)
    assert L.gvec_reward_config_default(None) == -1


def test_entry_point_refuses_bad_arguments_before_it_looks_at_the_handle():
    """Every refusal below happens with a NULL handle: the checks of the arguments themselves come first, so they hold on a box
    without a GPU; no call here can launch anything."""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import RewardConfigC
    L = g.load()
    fn = L.gvec_experience_rewards_config
    out = C.c_void_p(64)                                   # stands for an output array; never reached

    def refused(cfg, players, rewards, text):
        assert fn(None, None if cfg is None else C.byref(cfg), players, None, rewards, None, None, 1) == -1
        msg = L.gvec_last_error().decode()
        assert msg.startswith("gvec_experience_rewards_config") and text in msg, msg

    good = lambda: g.RewardConfig.go_default().to_c()      # noqa: E731
    refused(None, 0, out, "cfg is NULL")
    for field, _ in RewardConfigC._fields_[:10]:
        for bad in (float("nan"), float("inf"), -float("inf")):
            c = good()
            setattr(c, field, bad)
            refused(c, 0, out, f"{field} is not finite")
    c = good()
    c.reserved = 1
    refused(c, 0, out, "reserved must be 0")
    c = good()
    c.flags = 2
    refused(c, 0, out, "unknown flag bits")
    refused(good(), 0, None, "all NULL")
    refused(good(), 1 << 8, out, "at or above")
    refused(good(), 1, out, "handle is NULL")
    assert L.gvec_experience_begin_rewards(None) == -1


def test_envs_refuse_a_wrong_reward_config_before_they_need_a_device():
    import generalsreinforcementlearning_amd.selfplay_env as SE
    import generalsreinforcementlearning_amd.vector_env as VE
    for cls in (VE.GeneralsVecEnv, SE.GeneralsSelfPlayVecEnv):
        with pytest.raises(ValueError, match="reward_config must be a RewardConfig"):
            cls(4, 8, 8, reward_config="go")
