#!/usr/bin/env python3
"""Generates tests/golden/gym_env_fixtures.json - runs in the BUILD container only (it reads a checkout of the reference).

What it pins: everything the reference's own `GeneralsEnv` (python/generals_gym/generals_env.py, loaded as it lies, never
copied) does to a GameState proto - observation, valid-action mask, action decoding, reward, turn count, terminated /
truncated, the refusal returns, the info keys and their Python types.  What it does NOT pin: the Go server behind the
class; the server here is a fake whose state is the CPU oracle and whose GameState is wire.game_state, serialised and
re-parsed by the reference's generated stubs.

How the class is made to run without gymnasium and without a socket:
  * a stand-in `gymnasium` module (Env, register, spaces.Box, spaces.Discrete) goes into sys.modules before the import;
  * the loaded module's `time` is replaced by an object whose sleep() returns at once;
  * `_connect_to_server` is replaced: the stub is the fake; grpc.insecure_channel raises if anything reaches it.
The fake server: JoinGame hands out player ids 0 then 1; SubmitAction validates the move at submit time as
action_validator.go:114-139 does (the oracle's Validate) and raises a grpc.RpcError subclass on refusal; the turn is played
when the learner's GetGameState follows its accepted submit; an opponent that submitted nothing does not move.

Recorded (see tests/_gym_env_fixtures.py for the JSON form of an observation):
  (a) episodes against the reference's own `_submit_random_opponent_action` (random.seed fixed);
  (b) episodes whose `opponent_agent` returns the oracle agent's move for seat 1 from agent_actions(seed + 1000 k + 1),
      k = the step number counting refused steps (GeneralsVecEnv._step_device's schedule), at a recorded env index;
  (c) `_get_observation`, `_get_valid_actions_mask`, `_action_index_to_game_action`, `_calculate_reward` called on
      `GeneralsEnv.__new__` objects for every seat of 3- and 4-player games, dead viewers and eliminations included.

    python tests/golden/make_gym_env_fixtures.py [--out PATH]
"""
import ctypes as C
import importlib.util
import json
import logging
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GRL_REFERENCE_DIR", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "python"))

import _gym_env_fixtures as F  # noqa: E402
import _harness as H  # noqa: E402
import _oracle as O  # noqa: E402
from generalsreinforcementlearning_amd import wire  # noqa: E402

AGENT_SEED = 7
MAX_BYTES = 195192          # the largest fixture committed before this one (stream_client_fixtures.json)


# ---- the reference class, loaded as it lies --------------------------------------------------------------------------
def load_reference():
    gym = types.ModuleType("gymnasium")
    spaces = types.ModuleType("gymnasium.spaces")

    class Env:
        def reset(self, seed=None, options=None):
            pass

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, shape, dtype

    class Discrete:
        def __init__(self, n):
            self.n = int(n)

    gym.Env, gym.register, gym.spaces = Env, (lambda **kw: None), spaces
    spaces.Box, spaces.Discrete = Box, Discrete
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, spaces
    import grpc

    def no_channel(*a, **kw):
        raise AssertionError("the recorder opens no socket")
    grpc.insecure_channel = no_channel
    spec = importlib.util.spec_from_file_location("reference_generals_env", os.path.join(REF, "python", "generals_gym", "generals_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.time = types.SimpleNamespace(sleep=lambda s: None)
    logging.getLogger("GeneralsEnv").disabled = True        # the class logs every refused submit
    return mod


class Refused(Exception):
    pass


def refused_type(grpc):
    class RefusedRpc(grpc.RpcError, Refused):
        def __init__(self, msg):
            super().__init__(msg)
            self.msg = msg

        def code(self):
            return grpc.StatusCode.INVALID_ARGUMENT

        def details(self):
            return self.msg
    return RefusedRpc


class FakeServer:
    """CreateGame / JoinGame / SubmitAction / GetGameState on one env of an OracleBatch (the env index matters to the
    oracle agent's draw alone; every env of the batch holds the same board)."""

    def __init__(self, mod, w, h, fog, army, owner, typ, env=0, players=2):
        self.pb, self.w, self.h, self.fog, self.e, self.P = mod.game_pb2, w, h, fog, env, players
        self.Refused = refused_type(mod.grpc)
        n = env + 1
        self.ora = O.OracleBatch(n, w, h, players, fog=fog)
        self.ora.reset(np.tile(army, (n, 1)), np.tile(owner, (n, 1)), np.tile(typ, (n, 1)), [w] * n, [h] * n, [players] * n)
        self.joined, self.pending, self.turn_due, self.log = 0, {}, False, {}

    def CreateGame(self, req):
        cfg = req.config
        assert (cfg.width, cfg.height, cfg.max_players, cfg.fog_of_war) == (self.w, self.h, self.P, self.fog)
        return self.pb.CreateGameResponse(game_id="recorded-game")

    def JoinGame(self, req):
        pid = self.joined
        self.joined += 1
        return self.pb.JoinGameResponse(player_id=pid, player_token=f"token-{pid}")

    def SubmitAction(self, req):
        p, a = int(req.player_token.split("-")[1]), req.action
        src = getattr(a, "from")
        mv = O.Move(p, src.x, src.y, a.to.x, a.to.y, 0 if a.half else 1)
        board = self.ora.L.ora_engine_board(self.ora.engine(self.e).e)
        err = self.ora.L.ora_validate(board, C.byref(mv), p)
        if err:
            raise self.Refused(f"move refused by the validator: {err}")
        self.pending[p] = (src.x, src.y, a.to.x, a.to.y, bool(a.half))
        if p == 0:
            self.turn_due = True
        return self.pb.SubmitActionResponse(success=True)

    def play(self, moves):
        acts = np.zeros((self.ora.B, self.P), O.ACTION_DTYPE)
        for p, (fx, fy, tx, ty, half) in moves.items():
            acts[self.e, p] = (fx, fy, tx, ty, 1 | (2 if half else 0), (0, 0, 0))
        self.ora.step(acts)

    def state_for(self, p):
        st = self.ora.read_state(env_begin=self.e, n=1, fields=wire.STATE_FIELDS)
        eng = self.ora.engine(self.e)
        vis, fog = eng.player_visibility(p)
        gs = wire.game_state(st, vis[None], fog[None], eng.legal_mask(p), 0, p, game_id="recorded-game",
                             names=["RL_Agent", "Opponent"] + [f"player{q}" for q in range(2, self.P)])
        return self.pb.GameState.FromString(gs.SerializeToString())       # through the reference's own stubs

    def GetGameState(self, req):
        p = int(req.player_token.split("-")[1])
        if p == 0 and self.turn_due:
            self.play(self.pending)
            self.log, self.pending, self.turn_due = self.pending, {}, False
        return self.pb.GetGameStateResponse(state=self.state_for(p))


def make_env(mod, fake, **kw):
    mod.GeneralsEnv._connect_to_server = lambda self: setattr(self, "stub", fake)
    return mod.GeneralsEnv(**kw)


class AgentOpponent:
    """(b): the project's agent as the reference's `opponent_agent`."""

    def __init__(self, mod, fake):
        self.mod, self.fake, self.k = mod, fake, 0

    def select_action(self, state):
        a = self.fake.ora.agent_actions(AGENT_SEED + 1000 * self.k + 1)[self.fake.e, 1]
        if not (a["flags"] & 1):
            return None
        pb, cpb = self.mod.game_pb2, self.mod.common_pb2
        act = pb.Action(type=cpb.ACTION_TYPE_MOVE, half=bool(a["flags"] & 2))
        getattr(act, "from").CopyFrom(cpb.Coordinate(x=int(a["from_x"]), y=int(a["from_y"])))
        act.to.CopyFrom(cpb.Coordinate(x=int(a["to_x"]), y=int(a["to_y"])))
        return act


# ---- boards --------------------------------------------------------------------------------------------------------------
def generated(seed, w, h, players=2, general_army=None, block_first_dir=False):
    """A generated board; general_army: the learner's general starts with that army; block_first_dir: a mountain on the
    tile the half-move rule picks from the learner's general (up, or right in row 0) - the server-refused half move."""
    army, owner, typ, _, _, _ = H.gen_boards(seed, [(w, h, players)], w, h)
    army, owner, typ = army[0].copy(), owner[0].copy(), typ[0].copy()
    g = int(np.flatnonzero((typ == 1) & (owner == 0))[0])
    if general_army:
        army[g] = general_army
    if block_first_dir:
        dx, dy = F.DIRS[F.first_inboard_dir(g, w, h)]
        t = (g // w + dy) * w + g % w + dx
        assert typ[t] != 1
        army[t], owner[t], typ[t] = 0, -1, 3
    return army, owner, typ


def built(w, h, tiles):
    return O.planes_from_tiles(w, h, [dict(zip(("x", "y", "owner", "army", "type"), t)) for t in tiles])


N_, G_, C_, M_ = 0, 1, 2, 3     # core tile types


def endgame_win(w, h):          # a learner army next to the enemy general
    return built(w, h, [(0, 0, 0, 5, G_), (w - 2, h - 1, 0, 30, N_), (w - 1, h - 1, 1, 3, G_), (3, 2, -1, 40, C_), (2, 2, -1, 0, M_)])


def endgame_loss(w, h):         # the reverse: the opponent's only move takes the learner's general
    return built(w, h, [(w - 1, h - 1, 1, 50, G_), (w - 1, h - 2, -1, 0, M_), (w - 2, h - 1, 0, 2, G_), (0, 0, 0, 5, N_), (1, 0, 0, 1, N_),
                        (3, 3, -1, 40, C_)])


def lose_a_tile(w, h):          # the opponent's only move takes a learner tile: a negative tile delta
    return built(w, h, [(w - 1, h - 1, 1, 50, G_), (w - 1, h - 2, -1, 0, M_), (w - 2, h - 1, 0, 1, N_), (0, 0, 0, 5, G_), (1, 0, 0, 1, N_),
                        (4, 4, -1, 45, C_)])


# ---- recording -----------------------------------------------------------------------------------------------------------
def learner_stats(env):
    me = [p for p in env.current_state.players if p.id == env.player_id][0]
    return [int(me.tile_count), int(me.army_count)]


def record_return(env, obs, reward, terminated, truncated, info):
    assert isinstance(reward, float) and type(terminated) is bool and type(truncated) is bool
    return {"obs": F.encode_obs(obs), "mask": [int(i) for i in np.flatnonzero(env.valid_actions_mask)], "reward": reward.hex(),
            "terminated": terminated, "truncated": truncated, "info": F.encode_info(info), "stats": learner_stats(env)}


def choose(env, kind, rng, w, h):
    """The learner's action of one step.  kind: full / half / refuse / refuse_half / error (general's half move)."""
    mask = env.valid_actions_mask
    n = w * h
    if kind == "full":
        idx = [i for i in np.flatnonzero(mask) if i % 5 != 4]
    elif kind == "half":
        idx = [t * 5 + 4 for t in range(n) if mask[t * 5 + 4] and mask[t * 5 + F.first_inboard_dir(t, w, h)]]
        idx = [i for i in idx if F.first_inboard_dir(i // 5, w, h) != 0] or idx          # row 0 first: the rule's second direction
    elif kind == "refuse":
        idx = [i for i in np.flatnonzero(~mask) if i % 5 != 4]
    elif kind == "refuse_half":
        idx = [i for i in np.flatnonzero(~mask) if i % 5 == 4]
    else:
        idx = [t * 5 + 4 for t in range(n) if mask[t * 5 + 4] and not mask[t * 5 + F.first_inboard_dir(t, w, h)]]
    if not idx:
        return choose(env, "full", rng, w, h)
    return int(idx[rng.integers(0, len(idx))])


def record_episode(mod, name, kind, w, h, board, plan, fog=True, max_turns=500, env_index=0, seed=0):
    """plan: per step an action index, a (x, y, direction) move or a kind for `choose`."""
    army, owner, typ = board
    fake = FakeServer(mod, w, h, fog, army, owner, typ, env=env_index)
    agent = AgentOpponent(mod, fake) if kind == "b" else None
    env = make_env(mod, fake, board_width=w, board_height=h, max_players=2, fog_of_war=fog, max_turns=max_turns, opponent_agent=agent)
    random.seed(seed)                                   # the reference's random opponent draws from `random`
    rng = np.random.default_rng(seed)
    obs, info = env.reset()
    assert env.player_id == 0 and env.opponent_id == 1
    game = {"name": name, "kind": kind, "w": w, "h": h, "fog": fog, "max_turns": max_turns, "env": env_index, "seed": seed,
            "army": army.tolist(), "owner": owner.tolist(), "type": typ.tolist(),
            "reset": {"obs": F.encode_obs(obs), "mask": [int(i) for i in np.flatnonzero(info["valid_actions_mask"])],
                      "info": F.encode_info(info), "stats": learner_stats(env)}, "steps": []}
    for k, what in enumerate(plan):
        if isinstance(what, tuple):
            action = (what[1] * w + what[0]) * 5 + what[2]
        else:
            action = what if isinstance(what, int) else choose(env, what, rng, w, h)
        sent = env._action_index_to_game_action(action)           # the reference's decoding of this index (None: refused)
        if agent:
            agent.k = k
        fake.log = {}
        ret = env.step(action)
        step = {"action": action, "opponent": list(fake.log[1]) if 1 in fake.log else None,
                "sent": None if sent is None else [getattr(sent, "from").x, getattr(sent, "from").y, sent.to.x, sent.to.y, bool(sent.half)]}
        step.update(record_return(env, *ret))
        step["turn_count"] = env.turn_count
        game["steps"].append(step)
        if ret[2] or ret[3]:
            break
    return game


def mixed_plan(n, refuse=(), refuse_half=(), half=(), error=()):
    return ["refuse" if k in refuse else "refuse_half" if k in refuse_half else "half" if k in half else "error" if k in error else "full"
            for k in range(n)]


def record_episodes(mod):
    R, D, L, U = 1, 2, 3, 0
    eps = []
    # (a): the reference's own random opponent
    eps.append(record_episode(mod, "a_7x5", "a", 7, 5, generated(101, 7, 5, general_army=1500, block_first_dir=True),
                              mixed_plan(22, refuse=(2, 9), refuse_half=(5,), half=(3, 7, 12, 16), error=(1, 10)), env_index=0, seed=3))
    eps.append(record_episode(mod, "a_8x8", "a", 8, 8, generated(102, 8, 8, general_army=40, block_first_dir=True),
                              mixed_plan(20, refuse=(1, 8), refuse_half=(4,), half=(2, 6, 11), error=(3, 13)), env_index=0, seed=4))
    eps.append(record_episode(mod, "a_7x5_win", "a", 7, 5, endgame_win(7, 5), [(0, 0, R), "refuse", (5, 4, R), "full", "full"], env_index=33, seed=5))
    eps.append(record_episode(mod, "a_7x5_win_at_the_turn_limit", "a", 7, 5, endgame_win(7, 5), [(0, 0, R), (5, 4, R), "full"], max_turns=3, env_index=0, seed=5))
    eps.append(record_episode(mod, "a_8x8_loss", "a", 8, 8, endgame_loss(8, 8), [(0, 0, R), "full", "full", "full"], env_index=33, seed=6))
    eps.append(record_episode(mod, "a_8x8_loses_a_tile", "a", 8, 8, lose_a_tile(8, 8), [(0, 0, R), "full", "full", "full"], env_index=50, seed=7))
    eps.append(record_episode(mod, "a_8x8_fog_off_truncated", "a", 8, 8, generated(103, 8, 8), mixed_plan(8, refuse=(2,), half=(4,)), fog=False, max_turns=6,
                              env_index=0, seed=8))
    eps.append(record_episode(mod, "a_15x15", "a", 15, 15, generated(104, 15, 15, general_army=20, block_first_dir=True),
                              mixed_plan(10, refuse=(2,), half=(4,), error=(6,)), env_index=0, seed=9))
    eps.append(record_episode(mod, "a_20x20", "a", 20, 20, generated(105, 20, 20, general_army=20), mixed_plan(8, refuse_half=(3,), half=(5,)), env_index=0, seed=10))
    # (b): the project's agent in seat 1, at the env index of the replay
    eps.append(record_episode(mod, "b_7x5", "b", 7, 5, generated(111, 7, 5, general_army=9), mixed_plan(18, refuse=(12,), half=(14,)), env_index=17, seed=11))
    eps.append(record_episode(mod, "b_8x8", "b", 8, 8, generated(112, 8, 8, general_army=9), mixed_plan(18, refuse=(11,), half=(13,)), env_index=17, seed=12))
    eps.append(record_episode(mod, "b_15x15", "b", 15, 15, generated(113, 15, 15, general_army=9), mixed_plan(9, refuse=(7,)), env_index=33, seed=13))
    eps.append(record_episode(mod, "b_20x20", "b", 20, 20, generated(114, 20, 20, general_army=9), mixed_plan(8, refuse=(7,)), env_index=33, seed=14))
    return eps


# ---- (c): the pure methods on __new__ objects, every seat of 3- and 4-player games ----------------------------------------
def seat_object(mod, w, h, seat, max_turns):
    env = mod.GeneralsEnv.__new__(mod.GeneralsEnv)
    env.board_width, env.board_height, env.board_size, env.max_turns, env.player_id = w, h, w * h, max_turns, seat
    env.action_space = sys.modules["gymnasium.spaces"].Discrete(w * h * 5)
    return env


def record_multi(mod, name, w, h, P, board, scripted, turns, seed, max_turns=40, fog=True):
    """scripted: {turn: {seat: (x, y, direction)}}; every other move of a living seat is a seeded choice among its valid full
    moves that take no general.  Every living seat moves every turn (the self-play kernel's refusal penalty stays out)."""
    army, owner, typ = board
    fake = FakeServer(mod, w, h, fog, army, owner, typ, players=P)
    seats = [seat_object(mod, w, h, p, max_turns) for p in range(P)]
    rng = np.random.default_rng(seed)

    def look(k):
        views = []
        for p, s in enumerate(seats):
            s.current_state, s.turn_count = fake.state_for(p), k
            s.valid_actions_mask = s._get_valid_actions_mask()
            views.append({"obs": F.encode_obs(s._get_observation()), "mask": [int(i) for i in np.flatnonzero(s.valid_actions_mask)]})
        return views

    game = {"name": name, "w": w, "h": h, "players": P, "fog": fog, "max_turns": max_turns, "army": army.tolist(), "owner": owner.tolist(),
            "type": typ.tolist(), "views": look(0), "turns": []}
    for k in range(turns):
        alive = [pl.status == mod.common_pb2.PLAYER_STATUS_ACTIVE for pl in seats[0].current_state.players]
        true_type = fake.ora.read_state(fields=("type",))["type"][0]
        actions, decoded, moves = [], [], {}
        for p, s in enumerate(seats):
            if not alive[p]:
                actions.append(None), decoded.append(None)
                continue
            if p in scripted.get(k, {}):
                x, y, d = scripted[k][p]
                a = (y * w + x) * 5 + d
            else:
                ok = []
                for i in np.flatnonzero(s.valid_actions_mask):
                    t, d = divmod(int(i), 5)
                    if d < 4 and true_type[(t // w + F.DIRS[d][1]) * w + t % w + F.DIRS[d][0]] != 1:
                        ok.append(int(i))
                assert ok, (name, k, p)
                a = ok[rng.integers(0, len(ok))]
            act = s._action_index_to_game_action(a)
            assert act is not None, (name, k, p, a)
            src = getattr(act, "from")
            actions.append(a), decoded.append([src.x, src.y, act.to.x, act.to.y, bool(act.half)])
            moves[p] = tuple(decoded[-1])
        prev = [s.current_state for s in seats]
        fake.play(moves)
        views = look(k + 1)
        assert seats[0].current_state.status == mod.common_pb2.GAME_STATUS_IN_PROGRESS, (name, k)
        rewards = [s._calculate_reward(prev[p], s.current_state) for p, s in enumerate(seats)]
        assert all(isinstance(r, float) for r in rewards)
        now = [pl.status == mod.common_pb2.PLAYER_STATUS_ACTIVE for pl in seats[0].current_state.players]
        game["turns"].append({"actions": actions, "decoded": decoded, "views": views, "rewards": [r.hex() for r in rewards],
                              "alive": now, "eliminated": sum(a and not b for a, b in zip(alive, now))})
    return game


def record_multis(mod):
    U, R, D, L = 0, 1, 2, 3
    # 5x5, four generals in the corners; at turn 2 seat 0 takes seat 1's general and seat 2 takes seat 3's: two eliminations
    b5 = built(5, 5, [(0, 0, 0, 3, G_), (4, 0, 1, 2, G_), (0, 4, 2, 3, G_), (4, 4, 3, 2, G_), (2, 0, 0, 30, N_), (2, 4, 2, 30, N_),
                      (2, 2, -1, 0, M_), (1, 2, -1, 12, C_)])
    g5 = record_multi(mod, "c_5x5_p4", 5, 5, 4, b5, {0: {0: (2, 0, R), 2: (2, 4, R)}, 1: {0: (3, 0, R), 2: (3, 4, R)}}, 13, seed=21)
    # 10x10, three players; seat 0 takes seat 2's general at turn 3: one elimination, the game goes on
    b10 = built(10, 10, [(1, 1, 0, 4, G_), (8, 1, 1, 4, G_), (1, 8, 2, 2, G_), (1, 5, 0, 60, N_), (8, 2, 1, 1200, N_), (4, 4, -1, 40, C_),
                         (5, 4, -1, 0, M_), (5, 5, -1, 0, M_), (6, 7, -1, 44, C_), (0, 3, -1, 0, M_), (9, 9, -1, 0, M_), (3, 8, -1, 0, M_)])
    g10 = record_multi(mod, "c_10x10_p3", 10, 10, 3, b10, {0: {0: (1, 5, D)}, 1: {0: (1, 6, D)}, 2: {0: (1, 7, D)}}, 12, seed=22)
    return [g5, g10]


def build():
    mod = load_reference()
    fx = {"comment": "recorded by tests/golden/make_gym_env_fixtures.py from the reference's GeneralsEnv "
                     "(python/generals_gym/generals_env.py) over a fake server whose state is the CPU oracle; do not edit",
          "agent_seed": AGENT_SEED, "num_envs": F.NUM_ENVS, "episodes": record_episodes(mod), "multi": record_multis(mod)}
    # the recorder decodes what it encoded (encode_obs is checked against decode_obs on every observation it stores)
    for g in fx["episodes"]:
        for s in [g["reset"]] + g["steps"]:
            assert F.encode_obs(F.decode_obs(s["obs"], g["w"], g["h"])) == s["obs"]
    for g in fx["multi"]:
        for views in [g["views"]] + [t["views"] for t in g["turns"]]:
            for v in views:
                assert F.encode_obs(F.decode_obs(v["obs"], g["w"], g["h"])) == v["obs"]
    cov = F.coverage(fx)
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    assert sorted(t["eliminated"] for g in fx["multi"] for t in g["turns"] if t["eliminated"]) == [1, 2]
    assert all(len(g["turns"]) >= 12 and not all(g["turns"][-1]["alive"]) for g in fx["multi"])
    return fx


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "gym_env_fixtures.json")
    fx = build()
    text = json.dumps(fx, separators=(",", ":")) + "\n"
    assert json.loads(text) == fx and len(text) <= MAX_BYTES, len(text)
    with open(out, "w") as f:
        f.write(text)
    print(f"wrote {out}: {len(fx['episodes'])} episodes, {sum(len(g['steps']) for g in fx['episodes'])} steps, "
          f"{sum(len(g['turns']) for g in fx['multi'])} multi-player turns, {len(text)} bytes")


if __name__ == "__main__":
    main()
