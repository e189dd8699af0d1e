"""The engine and its board kernels held to the board's eight symmetries, on the device.

The rules do not know which way the board is turned: for every symmetry g of the rectangle (the flips, and the transposes
that swap an env's width and height), step(g.s, g.a) = g.step(s, a), field for field and bit for bit, for every output that
is a function of the board.  Each test deals a board and its images as separate envs of ONE padded, ragged batch, plays the
image of the base env's moves on every image env, and compares each image env with the transformed base env after every
turn.  No oracle is consulted for a single expected value: this is the device against itself, with the transforms of
tests/_equivariance.py (numpy; they share no index arithmetic and no direction table with the kernels).  The oracle only
supplies the base envs' moves, and tests/test_equivariance_reference.py asserts on it that these very runs hold aborted
turns, eliminations with tile turnover, finished games, growth turns, moves that share a tile and non-square boards under a
transpose.  A kernel breaks the property with adjacency across a row end, a fog neighbourhood that misses a corner, W where
H belongs, an edge tile on another code path, or an env's row pitch mixed up with the batch's - whether or not the oracle
shares the mistake.  What it cannot show is an error that is itself symmetric (wrong combat arithmetic): that is the lock-step
tests' business.

Every comparison is exact.

Excluded on purpose, because they are not symmetric BY DEFINITION (nobody should "fix" that):
  * gvec_bot_actions: among equally good moves the scripted opponent takes the lower source tile index;
  * the on-device random agent and the fused gvec_rollout: their draws are keyed by tile and env index;
  * the map generator, for the same reason (and the re-deal from the pool, keyed by env id: a gym pair is compared until it
    has been re-dealt).
So the moves here come from the host, and the gym envs' other seat is kept idle (GeneralsVecEnv) or is a learner too."""
import numpy as np
import pytest

import _oracle as O
import _state_forms as F
import test_equivariance_reference as R

pytestmark = pytest.mark.gpu


def _gpu():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def _twins(case):
    """the device engine under test and the oracle that moves the base envs, dealt the case's boards and their images"""
    g = _gpu()
    orb = R.Orbit(case)
    eng = g.VecEngine(orb.B, case["mw"], case["mh"], case["maxp"], fog_of_war=case["fog"])
    ora = O.OracleBatch(orb.B, case["mw"], case["mh"], case["maxp"], fog=case["fog"])
    orb.reset(eng)
    orb.reset(ora)
    ora.set_agent_mix(*case["mix"])
    return orb, eng, ora


# ---- (a) the step kernel and every per-player output, on every compiled variant -----------------------------------------------
@pytest.mark.parametrize("case", R.STEP_CASES + [R.FOG_OFF_CASE], ids=lambda c: c["id"])
def test_step_commutes_with_the_symmetries(case):
    """One launch steps every orientation side by side: err, game_state() and the packed legal masks every turn; observe(-1),
    the serializer mask, every player's visibility, the rewards (fixed weights and configured, after either snapshot) and the
    stream deltas every 5th turn."""
    orb, eng, ora = _twins(case)
    cov = R.drive(case, orb, eng, ora, case["turns"])
    R.assert_floors(cov, case)
    assert cov["rewards"] > 0 and cov["config_terms"] > 0
    eng.close()


# ---- (b) the aged forms: wide armies, lists that differ from ownership, turns next to a growth turn ---------------------------
@pytest.mark.parametrize("case", R.AGED_CASES, ids=lambda c: c["id"])
def test_step_commutes_with_the_symmetries_on_aged_envs(case):
    """The values of tests/_state_forms.py written through write_state into the base envs and, transformed, into their
    images: armies just below and above 65,535 (envs cross between the u16 and the int32 form in both directions), an owned
    tile its owner does not list, turns just before a multiple of 25; then the comparison of (a)."""
    orb, eng, ora = _twins(case)
    cov, tally = R.drive_aged(case, orb, eng, ora,
                              after_planting=lambda: F.check_flag_invariants(eng, eng.game_state(), f"{case['id']} after planting"))
    tally.assert_all_seen(case["id"])                   # wide and list-differs envs, and envs crossing in both directions
    assert cov["growth"] > 0 and cov["aborted"] > 0, cov
    F.check_flag_invariants(eng, eng.game_state(), f"{case['id']} at the end")
    eng.close()


# ---- (c) the gym kernels --------------------------------------------------------------------------------------------------------
def _deal(env, orb):
    """env.reset() (which builds the pool a re-deal draws from), then the case's boards in place of the generated ones and
    the reset-observe on them"""
    env.reset()
    env.engine.reset(*orb.boards)
    return env._to_numpy(*env._reset_device())


@pytest.mark.parametrize("name", list(R.GYM_CASES))
def test_gym_step_commutes_with_the_symmetries(name):
    """GeneralsVecEnv's one-launch gvec_gym_step, the other seat idle (an agent mix of nothing but no-ops: its draws are keyed
    by env index): observation, valid_actions_mask, reward to the bit, terminated, truncated."""
    _gpu()
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    orb = R.GymOrbit(name)
    env = GeneralsVecEnv(orb.B, board_width=orb.W, board_height=orb.H, max_players=2, max_turns=R.GYM_MAX_TURNS, seed=3, board_pool=16)
    env.engine.set_agent_mix(65536, 0)
    obs, info = _deal(env, orb)

    def step(actions):
        obs, reward, terminated, truncated, info = env.step(actions[:, 0])
        return obs[:, None], reward[:, None], terminated, truncated, info["valid_actions_mask"][:, None], info["turn"]

    seen = R.drive_gym(orb, step, obs[:, None], info["valid_actions_mask"][:, None], 1)
    R.assert_gym_floors(seen, name)
    env.close()


@pytest.mark.parametrize("name", list(R.GYM_CASES))
def test_selfplay_step_commutes_with_the_symmetries(name):
    """GeneralsSelfPlayVecEnv's gvec_gym_step_players with both seats learners: each learner's observation, mask and reward;
    the capture ends the game with +100 for one learner and -100 for the other."""
    _gpu()
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    orb = R.GymOrbit(name)
    env = GeneralsSelfPlayVecEnv(orb.B, board_width=orb.W, board_height=orb.H, max_players=2, max_turns=R.GYM_MAX_TURNS, seed=3, board_pool=16)
    obs, info = _deal(env, orb)

    def step(actions):
        obs, reward, terminated, truncated, info = env.step(actions)
        return obs, reward, terminated, truncated, info["valid_actions_mask"], info["turn"]

    seen = R.drive_gym(orb, step, obs, info["valid_actions_mask"], 2)
    R.assert_gym_floors(seen, name)
    env.close()
