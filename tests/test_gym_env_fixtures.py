"""The gym surface pinned by the reference's own GeneralsEnv class.

tests/golden/gym_env_fixtures.json holds what the reference's `GeneralsEnv` (python/generals_gym/generals_env.py) returned -
reset(), step() and its private helpers - when it ran in the build container over a fake server whose state is the CPU
oracle and whose GameState is wire.game_state re-parsed by the reference's stubs (tests/golden/make_gym_env_fixtures.py;
only the JSON travels).  Pinned: everything the Python class does to a GameState proto.  Not pinned: the Go server.

Tolerance is 0 throughout: observations are compared as uint32, rewards as uint64 (DESIGN.md section 5's parity bar).

CPU: the coverage conditions the fixture must meet; tests/_gym_reference.py's pure functions and NumpyReferenceVecEnv - the
checker every other gym test leans on - reproduce every recorded return; where a checkout of the reference exists the
fixture is recorded again and must come out byte for byte.
GPU: the gym kernels (gvec_gym_observe, gvec_gym_actions -> gvec_step -> gvec_gym_finish_step, gvec_gym_step, the *_players
kernels), GeneralsVecEnv and the single-env GeneralsEnv facade reproduce them in batches of 67 envs: the recorded games at
their env indices, seeded filler games around them."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _gym_env_fixtures as F
import _gym_reference as G
import _harness as H
import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "gym_env_fixtures.json")
with open(PATH) as f:
    FX = json.load(f)
GROUPS = F.groups(FX)
GROUP_IDS = {k: f"{k[0]}x{k[1]}_{'fog' if k[2] else 'nofog'}_max{k[3]}" for k in GROUPS}
PLAIN = [k for k in GROUPS if k[2] and k[3] == 500]                 # the four board sizes of the issue, fog on
SPECIAL = [k for k in GROUPS if k not in PLAIN]                      # fog off + truncation; the win at the turn limit
B = F.NUM_ENVS


@functools.lru_cache(maxsize=None)
def _want(kind, gi, k, seat=0):
    """(observation, mask) the reference returned: kind 'e' = episode gi, k = -1 reset / step k; 'm' = multi gi, k = -1 the
    initial views / turn k, for `seat`.  Decoded once, shared, read-only."""
    if kind == "e":
        g = FX["episodes"][gi]
        s = g["reset"] if k < 0 else g["steps"][k]
    else:
        g = FX["multi"][gi]
        s = (g["views"] if k < 0 else g["turns"][k]["views"])[seat]
    o, m = F.decode_obs(s["obs"], g["w"], g["h"]), F.decode_mask(s["mask"], g["w"], g["h"])
    o.setflags(write=False), m.setflags(write=False)
    return o, m


def _gi(g):
    return next(i for i, x in enumerate(FX["episodes"]) if x is g)


def _bits(r):
    return np.array([r], np.float64).view(np.uint64)[0]


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same_obs(got, want, ctx):
    got = np.ascontiguousarray(_np(got), np.float32).reshape(want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ctx, "observation", np.argwhere(got != want)[:6].tolist())


def _same_mask(got, want, ctx):
    got = _np(got).astype(bool).reshape(want.shape)
    assert np.array_equal(got, want), (ctx, "mask", np.flatnonzero(got != want)[:8].tolist())


def check_vec_step(ret, e, g, k, ctx):
    """One env of a vector step (GeneralsVecEnv / NumpyReferenceVecEnv return) against the reference's return of step k."""
    obs, reward, terminated, truncated, info = ret
    s, ctx = g["steps"][k], (ctx, g["name"], "env", e, "step", k)
    want_obs, want_mask = _want("e", _gi(g), k)
    _same_obs(_np(obs)[e], want_obs, ctx)
    _same_mask(_np(info["valid_actions_mask"])[e], want_mask, ctx)
    got_r = float(_np(reward)[e])
    assert _bits(got_r) == _bits(float.fromhex(s["reward"])), (ctx, "reward", got_r, float.fromhex(s["reward"]))
    assert bool(_np(terminated)[e]) == s["terminated"] and bool(_np(truncated)[e]) == s["truncated"], (ctx, "flags")
    ref = F.refusal(s)
    assert bool(_np(info["invalid_action"])[e]) == (ref == "invalid") and bool(_np(info["error"])[e]) == (ref == "error"), (ctx, "refusal", ref)
    assert int(_np(info["turn"])[e]) == s["turn_count"], (ctx, "turn")
    winner = s["info"]["winner"][0] if ref is None else None
    assert int(_np(info["winner"])[e]) == (-1 if winner is None else winner), (ctx, "winner")


# =====================================================================================================================
# CPU
# =====================================================================================================================
def test_fixture_meets_its_coverage_conditions():
    """Conditions, not measurements: the fixture cannot go hollow.  Every one is met by the episodes of kind (a) / (b)."""
    assert os.path.getsize(PATH) <= 195192, "no larger than the largest fixture committed before it"
    cov = F.coverage(FX)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    assert {(g["w"], g["h"]) for g in FX["episodes"]} == {(7, 5), (8, 8), (15, 15), (20, 20)}
    for kind in "ab":
        assert {(g["w"], g["h"]) for g in FX["episodes"] if g["kind"] == kind} == {(7, 5), (8, 8), (15, 15), (20, 20)}, kind
    small = sum(len(g["steps"]) for g in FX["episodes"] if g["w"] * g["h"] <= 64)
    assert small >= 40 and all(8 <= len(g["steps"]) <= 12 for g in FX["episodes"] if g["w"] >= 15)
    for key, games in GROUPS.items():
        assert all(0 <= g["env"] < B for g in games) and len({g["env"] for g in games}) == len(games), key
    for key in PLAIN:
        assert {0, B // 2, B - 1} <= set(F.place(GROUPS[key])), key
    # (c): 3 and 4 players, 5x5 and 10x10, >= 12 turns, one and two eliminations in one turn with the game going on, dead viewers
    multi = FX["multi"]
    assert {g["players"] for g in multi} == {3, 4} and {(g["w"], g["h"]) for g in multi} == {(5, 5), (10, 10)}
    assert all(len(g["turns"]) >= 12 for g in multi)
    assert sorted(t["eliminated"] for g in multi for t in g["turns"] if t["eliminated"]) == [1, 2]
    for g in multi:
        dead_turns = [t for t in g["turns"] if not all(t["alive"])]
        assert len(dead_turns) >= 5, g["name"]                       # states whose viewer is dead
        assert all(t["actions"].count(None) == prev.count(False) for prev, t in zip([[True] * g["players"]] + [t["alive"] for t in g["turns"]], g["turns"]))
    r50 = [float.fromhex(r) for g in multi for t in g["turns"] if t["eliminated"] for r in t["rewards"]]
    assert any(40 <= r < 90 for r in r50) and any(r >= 90 for r in r50), "the +50 term once and twice in one reward"


def _oracle_views(ora, e, w, h, players):
    st = ora.read_state(env_begin=e, n=1)
    out = []
    for p in range(players):
        vis, fog = ora.engine(e).player_visibility(p)
        out.append(G.proto_view(st["owner"], st["army"], st["type"], vis[None], fog[None]))
    return out, {f: st[f] for f in ("done", "winner", "alive", "army_count", "tile_count")}


def _move(acts, e, p, mv):
    fx, fy, tx, ty, half = mv
    acts[e, p] = (fx, fy, tx, ty, 1 | (2 if half else 0), (0, 0, 0))


def test_pure_functions_reproduce_every_recorded_step():
    """proto_view / build_observation / valid_actions_mask / decode_actions / calculate_reward on oracle states replayed from
    the recorded planes and moves, against the reference's return at every step of (a) and (b)."""
    for gi, g in enumerate(FX["episodes"]):
        w, h = g["w"], g["h"]
        ora = O.OracleBatch(1, w, h, 2, fog=g["fog"])
        army, owner, typ = F.planes(g)
        ora.reset(army[None], owner[None], typ[None], [w], [h], [2])
        views, stats = _oracle_views(ora, 0, w, h, 1)
        mask = G.valid_actions_mask(views[0], 0, w, h)[0]
        _same_obs(G.build_observation(views[0], 0, np.array([0]), g["max_turns"], w, h)[0], _want("e", gi, -1)[0], (g["name"], "reset"))
        _same_mask(mask, _want("e", gi, -1)[1], (g["name"], "reset"))
        assert g["reset"]["info"]["keys"] == ["game_id", "player_id", "turn", "valid_actions_mask"]
        assert g["reset"]["info"]["turn"] == [0, "int"] and g["reset"]["info"]["player_id"] == [0, "int"] and g["reset"]["info"]["game_id"][1] == "str"
        for k, s in enumerate(g["steps"]):
            ctx, a, ref = (g["name"], k), s["action"], F.refusal(s)
            fx_, fy, tx, ty, half, d = (int(v[0]) for v in G.decode_actions(np.array([a]), w, h))
            valid = bool(mask[a])
            accepted = valid and bool(mask[(fy * w + fx_) * 5 + d])            # NumpyReferenceVecEnv.step's two decisions
            assert (ref == "invalid") == (not valid) and (ref == "error") == (valid and not accepted), ctx
            assert (s["sent"] is None) == (not valid), ctx
            if valid:
                assert [fx_, fy, tx, ty, bool(half)] == s["sent"], (ctx, "decoded action")
            if ref is None:
                acts = np.zeros((1, 2), O.ACTION_DTYPE)
                _move(acts, 0, 0, s["sent"])
                if s["opponent"] is not None:
                    _move(acts, 0, 1, s["opponent"])
                ora.step(acts)
                prev = stats
                views, stats = _oracle_views(ora, 0, w, h, 1)
                mask = G.valid_actions_mask(views[0], 0, w, h)[0]
                r = float(G.calculate_reward(prev, stats, 0)[0])
                assert _bits(r) == _bits(float.fromhex(s["reward"])), (ctx, "reward", r)
                assert bool(stats["done"][0]) == s["terminated"] and (s["turn_count"] >= g["max_turns"]) == s["truncated"], ctx
                assert s["info"]["keys"] == ["game_status", "turn", "valid_actions_mask", "winner"], ctx
                assert s["info"]["turn"] == [s["turn_count"], "int"], ctx
                assert s["info"]["game_status"] == ["GAME_STATUS_FINISHED" if s["terminated"] else "GAME_STATUS_IN_PROGRESS", "str"], ctx
                assert s["info"]["winner"] == ([int(stats["winner"][0]), "int"] if s["terminated"] else [None, "NoneType"]), ctx
            else:
                assert float.fromhex(s["reward"]) == -0.1 and not s["terminated"] and not s["truncated"], ctx
                if ref == "invalid":
                    assert s["info"]["invalid_action"] == [True, "bool"], ctx
            assert [int(stats["tile_count"][0, 0]), int(stats["army_count"][0, 0])] == s["stats"], ctx
            _same_obs(G.build_observation(views[0], 0, np.array([s["turn_count"]]), g["max_turns"], w, h)[0], _want("e", gi, k)[0], ctx)
            _same_mask(mask, _want("e", gi, k)[1], ctx)


def test_pure_functions_reproduce_the_multi_player_vectors():
    """(c): every seat's observation and mask (dead viewers included), the decoded actions and the rewards (the +50 term for
    one and for two eliminations in a turn) of 3- and 4-player games."""
    for gi, g in enumerate(FX["multi"]):
        w, h, P = g["w"], g["h"], g["players"]
        ora = O.OracleBatch(1, w, h, P, fog=g["fog"])
        army, owner, typ = F.planes(g)
        ora.reset(army[None], owner[None], typ[None], [w], [h], [P])
        views, stats = _oracle_views(ora, 0, w, h, P)
        for k in range(-1, len(g["turns"])):
            if k >= 0:
                t = g["turns"][k]
                acts = np.zeros((1, P), O.ACTION_DTYPE)
                for p in range(P):
                    if t["actions"][p] is None:
                        assert not stats["alive"][0, p]
                        continue
                    assert G.valid_actions_mask(views[p], p, w, h)[0, t["actions"][p]], (g["name"], k, p)
                    dec = [int(v[0]) for v in G.decode_actions(np.array([t["actions"][p]]), w, h)][:5]
                    assert dec[:4] + [bool(dec[4])] == t["decoded"][p], (g["name"], k, p, "decoded action")
                    _move(acts, 0, p, t["decoded"][p])
                ora.step(acts)
                prev = stats
                views, stats = _oracle_views(ora, 0, w, h, P)
                assert [bool(v) for v in stats["alive"][0]] == t["alive"]
                for p in range(P):
                    r = float(G.calculate_reward(prev, stats, p)[0])
                    assert _bits(r) == _bits(float.fromhex(t["rewards"][p])), (g["name"], k, p, "reward", r)
            for p in range(P):
                want_obs, want_mask = _want("m", gi, k, p)
                _same_obs(G.build_observation(views[p], p, np.array([k + 1]), g["max_turns"], w, h)[0], want_obs, (g["name"], k, p))
                _same_mask(G.valid_actions_mask(views[p], p, w, h)[0], want_mask, (g["name"], k, p))


def _drive(env, key, reset_ret, step, compare_kinds, ctx, seed=5):
    """Plays a batch to the end of its longest recorded episode: recorded actions in recorded envs, a seeded masked-random
    policy in the fillers; `step(actions, k, at)` -> a vector step's return; episodes of `compare_kinds` are compared at
    every recorded step."""
    at = F.place(GROUPS[key])
    obs, info = reset_ret
    for e, g in at.items():
        _same_obs(_np(obs)[e], _want("e", _gi(g), -1)[0], (ctx, g["name"], "env", e, "reset"))
        _same_mask(_np(info["valid_actions_mask"])[e], _want("e", _gi(g), -1)[1], (ctx, g["name"], "env", e, "reset"))
        assert int(_np(info["turn"])[e]) == 0
    rng = np.random.default_rng(seed)
    compared = 0
    for k in range(max(len(g["steps"]) for g in at.values())):
        acts = F.learner_actions(_np(info["valid_actions_mask"]), at, k, rng)
        ret = step(acts, k, at)
        info = ret[4]
        for e, g in at.items():
            if k < len(g["steps"]) and g["kind"] in compare_kinds:
                check_vec_step(ret, e, g, k, ctx)
                compared += 1
    assert compared == sum(len(g["steps"]) for g in at.values() if g["kind"] in compare_kinds) > 0


def _oracle_env(key, maxp=2):
    from test_vector_env import OracleBackedEngine
    w, h, fog, max_turns = key
    env = G.NumpyReferenceVecEnv(OracleBackedEngine(B, w, h, maxp, fog_of_war=fog), B, w, h, max_players=maxp, fog_of_war=fog,
                                 max_turns=max_turns, seed=FX["agent_seed"], board_pool=16)
    env.reset()
    army, owner, typ, ws, hs, ps, _ = F.batch_planes(GROUPS[key], w, h)
    return env, env.install_boards(army, owner, typ, ws, hs, ps)


@pytest.mark.parametrize("key", list(GROUPS), ids=list(GROUP_IDS.values()))
def test_numpy_reference_env_reproduces_the_recorded_episodes(key):
    """NumpyReferenceVecEnv over the oracle - the checker every other gym test leans on - against the reference's returns,
    step for step: reward, terminated, truncated, turn, invalid_action, error, winner, observation and mask.  The recorded
    opponent moves are played in place of its own draw ((a) and (b)); then, with its own draw, the (b) episodes again."""
    env, reset_ret = _oracle_env(key)
    _drive(env, key, reset_ret, lambda acts, k, at: env.step(acts, other_actions=F.opponent_actions(O.ACTION_DTYPE, env.engine.agent_actions(900 + k), at, k, 2)),
           "ab", "supplied moves")
    if any(g["kind"] == "b" for g in GROUPS[key]):
        env, reset_ret = _oracle_env(key)
        _drive(env, key, reset_ret, lambda acts, k, at: env.step(acts), "b", "own draw")


def test_agent_draw_of_a_two_player_env_ignores_the_player_limit():
    """What lets the one-launch step be checked against the (b) episodes on handles of 4 and 8 players: the oracle agent's
    draw for a two-player env is the same whatever the batch's player limit."""
    key = next(k for k in PLAIN if k[:2] == (8, 8))
    army, owner, typ, ws, hs, ps, _ = F.batch_planes(GROUPS[key], 8, 8)
    oras = [O.OracleBatch(B, 8, 8, P) for P in (2, 4, 8)]
    for o in oras:
        o.reset(army, owner, typ, ws, hs, ps)
    for k in range(12):
        draws = [o.agent_actions(FX["agent_seed"] + 1000 * k + 1) for o in oras]
        assert draws[0]["flags"].any()
        for o, d in zip(oras, draws):
            assert np.array_equal(d[:, :2], draws[0]) and not d[:, 2:]["flags"].any(), k
            o.step(d)


def test_fixture_is_what_the_reference_records_today():
    """Where a checkout of the reference exists (GRL_REFERENCE_DIR, by default the build container's), the recorder runs
    again - in a process of its own: it puts a stand-in gymnasium into sys.modules - and must write the committed bytes."""
    ref = os.environ.get("GRL_REFERENCE_DIR", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "python", "generals_gym", "generals_env.py")):
        pytest.skip("no checkout of the reference here: the fixture is recorded in the build container only")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "again.json")
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_gym_env_fixtures.py"), "--out", out], check=True, env=env,
                       stdout=subprocess.DEVNULL, timeout=120)
        with open(out, "rb") as a, open(PATH, "rb") as b:
            assert a.read() == b.read(), "tests/golden/gym_env_fixtures.json is stale: run tests/golden/make_gym_env_fixtures.py"


# =====================================================================================================================
# GPU
# =====================================================================================================================
def _deal(env, pool_players, army, owner, typ, ws, hs, ps):
    """What env.reset() does, on the boards of the test: the pool a re-deal draws from, the boards, the reset-observe.  The
    pool's boards have `pool_players` seats, as the boards have, not the handle's player limit: the generator cannot space 4
    generals on every 7x5 board, nor 8 on any, and refuses (GVEC_E_BOARD) as the reference's generator does."""
    env.engine.build_board_pool(16, FX["agent_seed"] * 7919 + 5, players=np.full(16, pool_players, np.int32))
    env.engine.reset(army, owner, typ, ws, hs, ps)
    return env._reset_device()


def _hip_env(key, maxp=2, device_outputs=False):
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    w, h, fog, max_turns = key
    env = GeneralsVecEnv(B, board_width=w, board_height=h, max_players=maxp, fog_of_war=fog, max_turns=max_turns, seed=FX["agent_seed"],
                         board_pool=16, device_outputs=device_outputs)
    army, owner, typ, ws, hs, ps, _ = F.batch_planes(GROUPS[key], w, h)
    obs, info = _deal(env, 2, army, owner, typ, ws, hs, ps)
    return env, ((obs, info) if device_outputs else env._to_numpy(obs, info))


@pytest.mark.gpu
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("key", PLAIN + SPECIAL, ids=[GROUP_IDS[k] for k in PLAIN + SPECIAL])
def test_reset_observe_equals_the_references_reset(key, maxp):
    """gvec_gym_observe (the reset path) on imported boards: the reference's reset observation and mask, on every store path
    of gym_emit (one / four / seven slots, odd and even planes) and every register layout (handles of 2, 4, 8 players)."""
    env, (obs, info) = _hip_env(key, maxp)
    at = F.place(GROUPS[key])
    for e, g in at.items():
        _same_obs(obs[e], _want("e", _gi(g), -1)[0], (g["name"], "env", e))
        _same_mask(info["valid_actions_mask"][e], _want("e", _gi(g), -1)[1], (g["name"], "env", e))
    assert not _np(info["turn"]).any() and len(at) >= 1
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("maxp,device_outputs", [(2, False), (2, True), (4, True), (8, False)], ids=["p2_numpy", "p2_device", "p4_device", "p8_numpy"])
@pytest.mark.parametrize("key", list(GROUPS), ids=list(GROUP_IDS.values()))
def test_composed_step_equals_the_references_step(key, maxp, device_outputs):
    """GeneralsVecEnv.step(actions, other_actions=the recorded opponent moves) - gvec_gym_actions -> gvec_step ->
    gvec_gym_finish_step - at every recorded step of (a) and (b)."""
    import torch
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    env, reset_ret = _hip_env(key, maxp, device_outputs)

    def step(acts, k, at):
        others = F.opponent_actions(ACTION_DTYPE, env.engine.agent_actions(900 + k), at, k, maxp)
        return env.step(torch.from_numpy(acts).cuda() if device_outputs else acts, other_actions=others)
    _drive(env, key, reset_ret, step, "ab", f"composed p{maxp}")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("key", PLAIN, ids=[GROUP_IDS[k] for k in PLAIN])
def test_one_launch_step_equals_the_references_step(key, maxp):
    """gvec_gym_step (step(actions) with no other_actions: the opponent is the on-device agent) against the (b) episodes,
    whose opponent was the oracle's agent on the same schedule at the same env index.  Handles of 4 and 8 players too: the
    agent's draw for a two-player env does not depend on the handle's player limit
    (test_agent_draw_of_a_two_player_env_ignores_the_player_limit)."""
    env, reset_ret = _hip_env(key, maxp)
    _drive(env, key, reset_ret, lambda acts, k, at: env.step(acts), "b", f"one launch p{maxp}")
    env.close()


class _Replay:
    """An `opponent_agent` that replays the recorded opponent moves: one per step the reference asked its opponent for."""

    def __init__(self, g):
        self.moves = iter([s["opponent"] for s in g["steps"] if F.refusal(s) is None])
        self.asked = 0

    def select_action(self, state):
        self.asked += 1
        mv = next(self.moves)
        if mv is None:
            return None
        NS = types.SimpleNamespace
        return NS(**{"from": NS(x=mv[0], y=mv[1]), "to": NS(x=mv[2], y=mv[3]), "half": mv[4]})


@pytest.mark.gpu
@pytest.mark.parametrize("gi", [i for i, g in enumerate(FX["episodes"]) if g["kind"] == "a"],
                         ids=[g["name"] for g in FX["episodes"] if g["kind"] == "a"])
def test_single_env_facade_returns_the_references_five_tuple(gi):
    """The project's GeneralsEnv driven with a recorded (a) action sequence and an opponent_agent that replays the recorded
    moves: the reference's five-tuple at every step - the same info key set, the same Python types (winner None against int,
    turn int, reward float), the same game_status; a refused step is exactly (obs, -0.1, False, False, {"invalid_action":
    True}), a server-refused one carries the single key "error".  The opponent is asked exactly when the reference asks."""
    from generalsreinforcementlearning_amd.vector_env import GeneralsEnv
    g = FX["episodes"][gi]
    w, h = g["w"], g["h"]
    opp = _Replay(g)
    env = GeneralsEnv(board_width=w, board_height=h, max_players=2, fog_of_war=g["fog"], max_turns=g["max_turns"], opponent_agent=opp)
    obs, info = env.reset()
    want = g["reset"]["info"]
    assert sorted(info) == want["keys"] and all(type(info[k]).__name__ == want[k][1] for k in ("game_id", "player_id", "turn"))
    assert (info["player_id"], info["turn"]) == (want["player_id"][0], want["turn"][0])
    army, owner, typ = F.planes(g)                                      # the recorded board in place of the generated one
    env._vec.engine.reset(army[None], owner[None], typ[None], [w], [h], [2])
    o, i = env._vec._to_numpy(*env._vec._reset_device())
    env._obs, env.valid_actions_mask = o[0].copy(), i["valid_actions_mask"][0].copy()
    _same_obs(env._obs, _want("e", gi, -1)[0], (g["name"], "reset"))
    _same_mask(env.valid_actions_mask, _want("e", gi, -1)[1], (g["name"], "reset"))
    for k, s in enumerate(g["steps"]):
        ctx = (g["name"], k)
        obs, reward, terminated, truncated, info = env.step(s["action"])
        assert obs.dtype == np.float32 and type(reward) is float and type(terminated) is bool and type(truncated) is bool, ctx
        _same_obs(obs, _want("e", gi, k)[0], ctx)
        _same_mask(env.valid_actions_mask, _want("e", gi, k)[1], ctx)
        assert _bits(reward) == _bits(float.fromhex(s["reward"])) and (terminated, truncated) == (s["terminated"], s["truncated"]), (ctx, reward)
        want = s["info"]
        assert sorted(info) == want["keys"], (ctx, sorted(info))
        ref = F.refusal(s)
        if ref == "invalid":
            assert (reward, terminated, truncated, info) == (-0.1, False, False, {"invalid_action": True}), ctx
        elif ref == "error":
            assert (reward, terminated, truncated) == (-0.1, False, False) and list(info) == ["error"], ctx
        else:
            for key in ("turn", "game_status", "winner"):
                assert [info[key], type(info[key]).__name__] == want[key], (ctx, key, info[key])
            _same_mask(info["valid_actions_mask"], _want("e", gi, k)[1], ctx)
        assert env.turn_count == s["turn_count"], ctx
    assert opp.asked == sum(F.refusal(s) is None for s in g["steps"]) and next(opp.moves, "end") == "end"
    env.close()


def _selfplay_env(w, h, P, learners, fog, max_turns, army, owner, typ, ws, hs, ps):
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(B, board_width=w, board_height=h, max_players=P, learners=learners, fog_of_war=fog, max_turns=max_turns,
                                 seed=FX["agent_seed"], board_pool=16)
    return env, env._to_numpy(*_deal(env, int(min(ps)), army, owner, typ, ws, hs, ps))


@pytest.mark.gpu
@pytest.mark.parametrize("key", PLAIN, ids=[GROUP_IDS[k] for k in PLAIN])
def test_selfplay_kernel_with_one_learner_equals_the_references_step(key):
    """gvec_gym_step_players with learners = {0} on the prefix of a (b) episode that has no refused action (a refusal is where
    the self-play kernel differs on purpose): observation, mask, reward and flags of learner 0."""
    w, h, fog, max_turns = key
    army, owner, typ, ws, hs, ps, at = F.batch_planes(GROUPS[key], w, h)
    env, (obs, info) = _selfplay_env(w, h, 2, [0], fog, max_turns, army, owner, typ, ws, hs, ps)
    e, g = next((e, g) for e, g in at.items() if g["kind"] == "b")
    prefix = next((k for k, s in enumerate(g["steps"]) if F.refusal(s)), len(g["steps"]))
    assert prefix >= 6
    _same_obs(obs[e, 0], _want("e", _gi(g), -1)[0], (g["name"], "reset"))
    rng = np.random.default_rng(6)
    for k in range(prefix):
        s, ctx = g["steps"][k], (g["name"], "env", e, "step", k)
        acts = F.learner_actions(info["valid_actions_mask"][:, 0], {e: g}, k, rng)
        obs, reward, terminated, truncated, info = env.step(acts.reshape(B, 1))
        want_obs, want_mask = _want("e", _gi(g), k)
        _same_obs(obs[e, 0], want_obs, ctx)
        _same_mask(info["valid_actions_mask"][e, 0], want_mask, ctx)
        assert _bits(float(reward[e, 0])) == _bits(float.fromhex(s["reward"])), (ctx, float(reward[e, 0]))
        assert (bool(terminated[e]), bool(truncated[e])) == (s["terminated"], s["truncated"]) and int(info["turn"][e]) == s["turn_count"], ctx
        assert not info["invalid"][e, 0] and not info["error"][e, 0] and bool(info["alive"][e, 0]), ctx
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(FX["multi"])), ids=[g["name"] for g in FX["multi"]])
def test_players_kernels_equal_the_multi_player_vectors(gi):
    """(c) on the device: the recorded game at the first, a middle and the last env, fillers between.  After the import and
    after every recorded turn gvec_gym_observe(player) and gvec_gym_observe_players / gvec_gym_step_players (every seat a
    learner) give the reference's observation and mask per seat, dead viewers included; the step's reward per seat is
    `_calculate_reward`'s value (no recorded action is refused, so the self-play refusal penalty stays out)."""
    import torch
    from generalsreinforcementlearning_amd._lib import check
    g = FX["multi"][gi]
    w, h, P, n = g["w"], g["h"], g["players"], g["w"] * g["h"]
    fill = min(P, max(2, n // 30))
    army, owner, typ, ws, hs, ps = H.gen_boards(13, [(w, h, fill)] * B, w, h)
    where = (0, B // 2, B - 1)
    for e in where:
        (army[e], owner[e], typ[e]), ps[e] = F.planes(g), P
    env, (obs, info) = _selfplay_env(w, h, P, None, g["fog"], g["max_turns"], army, owner, typ, ws, hs, ps)
    one_obs = torch.zeros((B, 9, n), dtype=torch.float32, device="cuda")
    one_mask = torch.zeros((B, n * 5), dtype=torch.uint8, device="cuda")

    def compare(k):
        for p in range(P):
            check(env.engine.L.gvec_gym_observe(env.engine.h, p, env._d_turn.data_ptr(), g["max_turns"], one_obs.data_ptr(), one_mask.data_ptr(),
                                                None, None, None), "gvec_gym_observe")
            so, sm = one_obs.cpu().numpy(), one_mask.cpu().numpy()
            want_obs, want_mask = _want("m", gi, k, p)
            for e in where:
                ctx = (g["name"], "turn", k, "env", e, "seat", p)
                _same_obs(obs[e, p], want_obs, ctx + ("players kernel",))
                _same_mask(info["valid_actions_mask"][e, p], want_mask, ctx + ("players kernel",))
                _same_obs(so[e], want_obs, ctx + ("gvec_gym_observe",))
                _same_mask(sm[e], want_mask, ctx + ("gvec_gym_observe",))

    compare(-1)
    rng = np.random.default_rng(7)
    for k, t in enumerate(g["turns"]):
        m = info["valid_actions_mask"]
        acts = np.array([[int(rng.choice(np.flatnonzero(m[e, p]))) if m[e, p].any() else 0 for p in range(P)] for e in range(B)], np.int64)
        for e in where:
            acts[e] = [0 if a is None else a for a in t["actions"]]
        obs, reward, terminated, truncated, info = env.step(acts)
        compare(k)
        for e in where:
            for p in range(P):
                assert _bits(float(reward[e, p])) == _bits(float.fromhex(t["rewards"][p])), (g["name"], k, e, p, float(reward[e, p]), float.fromhex(t["rewards"][p]))
                assert bool(info["alive"][e, p]) == t["alive"][p] and not info["invalid"][e, p] and not info["error"][e, p], (g["name"], k, e, p)
            assert not terminated[e] and not truncated[e] and int(info["turn"][e]) == k + 1
    env.close()
