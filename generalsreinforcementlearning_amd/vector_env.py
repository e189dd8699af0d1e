"""GeneralsVecEnv — drop-in *vector* form of the reference's gym environment.

Reference: python/generals_gym/generals_env.py (GeneralsEnv) and vector_env.py (ParallelEnvPool,
which runs N GeneralsEnv instances from N threads, each doing two gRPC round trips and a 50 ms
sleep per step).  Here the same per-env interface is served for B boards by ONE HIP launch per
step (gvec_gym_step):

  * observation (9, H, W) float32            generals_env.py:111-116, 291-342
  * action space Discrete(board_size * 5)    generals_env.py:118-120, 344-387 (idx*5 + {up,right,down,left,half})
  * action decoding incl. the half-move quirk generals_env.py:389-441
  * reward                                    generals_env.py:499-561
  * terminated / truncated / info keys        generals_env.py:272-289

What the learner sees is the *proto* view the gRPC server would send for its player token:
fog rules of internal/grpc/gameserver/server.go:556-582 (hidden tile -> type NORMAL, owner -1,
army 0; fogged tile -> type kept, owner / army hidden) and the PlayerState fields of
server.go:526-553 (army_count = Player.ArmyCount, tile_count = len(OwnedTiles), status by Alive).

There is one execution path: the gym kernels behind the C ABI.  (The readable numpy restatement they
are tested against lives in tests/_gym_reference.py; it was a third mode of this class up to round 2.)

Deliberate differences (documented in DESIGN.md): opponents are by default the on-device random agent
(uniform over legal moves, 30 % half moves, 10 % no-op) instead of Python's `random.choice` over
full moves - or whatever the caller supplies per step (`step(actions, other_actions=...)`: an opponent
policy, self-play; GeneralsEnv's `opponent_agent`); finished / truncated envs are re-dealt on their next step ("next-step" autoreset)
because a vector env cannot wait for a per-env reset() call.

Buffers, reset / force_reset, numpy mode and the state methods are GymVecEnvBase's (_gym_base.py), shared with
GeneralsSelfPlayVecEnv; this file holds the opponent options and the three ways a step is launched.
"""
import numpy as np

from ._gym_base import GymVecEnvBase
from ._lib import check


class GeneralsVecEnv(GymVecEnvBase):
    """B GeneralsEnv instances behind the (gymnasium-style) vector API:
    reset() -> (obs, info);  step(actions[B]) -> (obs, reward, terminated, truncated, info).
    copy_envs / save_state / restore_state (_gym_base.py): clone, save and restore env states on the device."""
    _STEP_FLAGS = ("played", "invalid", "error")        # gvec_gym_step's last three outputs
    _INFO_FLAGS = (("invalid_action", "invalid"), ("error", "error"))

    def __init__(self, num_envs, board_width=15, board_height=15, max_players=2, fog_of_war=True, max_turns=500,
                 seed=0, device=0, board_pool=1024, device_outputs=False, opponent="random", opponent_random_permille=0,
                 strategic_features=False, feature_cap=64, reward_config=None):
        """device_outputs=True  observation / mask / reward / flags are torch tensors on the GPU; `step` takes a CUDA int64
                             tensor of actions: no board state crosses PCIe, a step is one kernel launch.  Every tensor a
                             step returns lives in a buffer that the step AFTER NEXT reuses.
        default              numpy arrays in, numpy arrays out - the same kernel, its outputs copied to pinned host
                             buffers (one D2H of the observation per step).
        opponent="random"    the other seats are the on-device random agent (one launch per step).
        opponent="bot"       the other seats are the scripted opponent (gvec_bot_actions), computed on
                             the device into the step's action buffer, then the composed step (_step_composed);
                             opponent_random_permille of its moves are the random agent's instead.
        step(actions, other_actions=...) overrides either choice for that step.
        strategic_features=True  (needs device_outputs=True) reset / step / copy_envs / restore_state add
                             info["strategic_features"], float32 [B, 5, H, W]: features.strategic_features of the observation
                             they return, distances capped at feature_cap.  One extra launch per call.
        reward_config=RewardConfig  `step`'s reward is the reference's CalculateRewardWithConfig with these weights
                             (reward.py) instead of GeneralsEnv._calculate_reward: two extra launches per step (a reward-only
                             snapshot before it, the rewards after it) on the same stream; a refused action - which this env
                             does not play - yields exactly config.invalid_action.  info["reward_terms"] (device mode):
                             int32 [B, 8].  Everything else a step returns is unchanged.  None: today's reward, no extra launch."""
        feat_cap = self._feature_option(strategic_features, feature_cap, device_outputs)
        reward_c = self._reward_option(reward_config)
        if opponent not in ("random", "bot"):
            raise ValueError(f"opponent must be 'random' or 'bot', not {opponent!r}")
        if not 0 <= int(opponent_random_permille) <= 1000:
            raise ValueError("opponent_random_permille must be in [0, 1000]")
        self._require_gpu()
        super().__init__((), feat_cap, num_envs, board_width, board_height, max_players, fog_of_war, max_turns, seed, device,
                         board_pool, device_outputs, reward_c)
        self.player_id = 0  # "RL_Agent" joins first (generals_env.py:163-169)
        self.opponent, self.opponent_random_permille = opponent, int(opponent_random_permille)
        self._acts = None

    # ---- the device path ---------------------------------------------------------------------------------
    def _observe_info(self):
        self._obs_flip ^= 1
        obs, mask = self._d_obs[self._obs_flip], self._d_mask[self._obs_flip]
        e = self.engine
        check(e.L.gvec_gym_observe(e.h, self.player_id, self._d_turn.data_ptr(), self.max_turns, obs.data_ptr(), mask.data_ptr(),
                                   self._d_reward.data_ptr(), self._d_done.data_ptr(), self._d_winner.data_ptr()), "gvec_gym_observe")
        self.valid_actions_mask = mask.view(self._t.bool)
        return obs, self._add_features(obs, {"player_id": self.player_id, "valid_actions_mask": self.valid_actions_mask,
                                             "turn": self._d_turn.clone()})

    def _learner_ids(self):
        return [self.player_id]

    def _step_device(self, actions):
        e = self.engine
        self.last_actions = actions = self._as_actions(actions)        # the tensor the launch reads (kept alive; a collector records it)
        self._reward_begin()
        k = self._step_no
        self._step_no += 1
        self._obs_flip ^= 1
        ptrs, obs, out, info = self._step_args(k, self._obs_flip)
        # ONE launch: the learner's action decoded against the resident state's mask (`resetting` = the needs_reset the previous
        # step wrote, zeroed by reset, raised by force_reset), the opponents' moves from the on-device agent, the turn, then
        # observation / mask / reward / flags of the new state (aborted turns are the opponents' business, as over gRPC)
        check(e.L.gvec_gym_step(e.h, self.player_id, self._seed + 1000 * self._episode + 1, actions.data_ptr(), *ptrs), "gvec_gym_step")
        self._episode += 1
        self.valid_actions_mask = info["valid_actions_mask"]
        return obs, out["reward"], out["terminated"], out["truncated"], self._reward_finish(out, self._add_features(obs, dict(info)))

    def _other_moves(self):
        """The [num_envs, max_players, 8] uint8 buffer of the composed step's gvec_action moves, made on first use."""
        if self._acts is None:
            self._acts = self._t.zeros((self.num_envs, self.max_players, 8), dtype=self._t.uint8, device=self._dev)
        return self._acts

    def _step_bot(self, actions):
        """The other seats played by the scripted opponent: gvec_bot_actions writes their moves into the step's action buffer
        on the device (seeded like the random agent's draw of a one-launch step), then the composed step runs on it."""
        others = ((1 << self.max_players) - 1) & ~(1 << self.player_id)
        self.engine.bot_actions_device(others, self._seed + 1000 * self._episode + 1, self.opponent_random_permille,
                                       self._other_moves().data_ptr())
        self._episode += 1
        return self._step_composed(actions, None)

    def _step_composed(self, actions, others):
        """The same step with the OTHER players' moves supplied by the caller - an opponent policy, self-play - instead of
        drawn by the on-device agent: `others` is [num_envs][max_players] gvec_action (numpy ACTION_DTYPE, or a CUDA uint8
        tensor [num_envs, max_players, 8]); the learner's slot is ignored.  Four launches - gvec_gym_actions (the learner's
        action decoded into its slot, a refused one makes the env sit the call out) -> gvec_step -> gvec_gym_finish_step -
        which together equal gvec_gym_step output for output when `others` are the agent's moves
        (tests/test_vector_env.py::test_gym_step_equals_the_four_call_composition)."""
        t, e, B, P = self._t, self.engine, self.num_envs, self.max_players
        actions, acts = self._as_actions(actions), self._other_moves()
        if isinstance(others, np.ndarray):
            from .vec_engine import ACTION_DTYPE
            others = t.from_numpy(np.ascontiguousarray(others, ACTION_DTYPE).reshape(B, P).view(np.uint8).reshape(B, P, 8))
        if others is not None:                                          # None: acts already holds them (_step_bot)
            acts.copy_(others.reshape(B, P, 8))
        self.last_actions = actions
        k = self._step_no
        self._step_no += 1
        prev_mask = self._d_mask[self._obs_flip]                       # the mask of the observation the learner acted on
        self._obs_flip ^= 1
        _, obs, out, info = self._step_args(k, self._obs_flip)
        cur, mask = self._d_step[k % 3], self._d_mask[self._obs_flip]
        L, pl = e.L, self.player_id
        self._reward_begin()
        check(L.gvec_gym_actions(e.h, pl, actions.data_ptr(), prev_mask.data_ptr(), cur["needs_reset"].data_ptr(), acts.data_ptr(),
                                 out["played"].data_ptr(), out["invalid"].data_ptr(), out["error"].data_ptr()), "gvec_gym_actions")
        e.step_device(acts.data_ptr())
        check(L.gvec_gym_finish_step(e.h, pl, self._d_turn.data_ptr(), self.max_turns, cur["needs_reset"].data_ptr(), out["played"].data_ptr(),
                                     obs.data_ptr(), mask.data_ptr(), out["reward"].data_ptr(), out["terminated"].data_ptr(),
                                     out["truncated"].data_ptr(), out["winner"].data_ptr(), out["needs_reset"].data_ptr(),
                                     out["turn"].data_ptr()), "gvec_gym_finish_step")
        self.valid_actions_mask = info["valid_actions_mask"]
        return obs, out["reward"], out["terminated"], out["truncated"], self._reward_finish(out, self._add_features(obs, dict(info)))

    # ---- gym API ------------------------------------------------------------------------------------
    def step(self, actions, other_actions=None):
        """other_actions: None = the other players are the env's opponent (the on-device random agent in ONE launch, or the
        scripted opponent with opponent="bot"); else their moves for this step ([num_envs][max_players] gvec_action, see
        _step_composed)."""
        if other_actions is not None:
            run = lambda a: self._step_composed(a, other_actions)
        else:
            run = self._step_bot if self.opponent == "bot" else self._step_device
        if self.device_outputs:
            return run(actions)
        return self._step_to_numpy(*run(np.asarray(actions, np.int64)))


# --------------------------------------------------------------------------------------------------------------------
# The single-env shape: what code written against the reference's `GeneralsEnv` (and its ParallelEnvPool, whose
# env_factory makes one env per worker) instantiates.  gymnasium is not a dependency of this package: the two spaces are
# minimal stand-ins with the attributes that code reads (.shape / .dtype / .low / .high, .n / .sample() / .contains()).
# --------------------------------------------------------------------------------------------------------------------
class _Box:
    def __init__(self, low, high, shape, dtype):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool((x >= self.low).all() and (x <= self.high).all())


class _Discrete:
    def __init__(self, n, seed=None):
        self.n = int(n)
        self._rng = np.random.default_rng(seed)

    def sample(self, mask=None):
        if mask is not None and np.any(mask):
            return int(self._rng.choice(np.flatnonzero(mask)))
        return int(self._rng.integers(self.n))

    def contains(self, x):
        return 0 <= int(x) < self.n


class GeneralsEnv:
    """python/generals_gym/generals_env.py:GeneralsEnv - same constructor keywords, `observation_space` (Box(0, 1,
    (9, H, W), float32), :111-116), `action_space` (Discrete(board_size * 5), :118-120), `reset(seed, options) -> (obs,
    info)` (:142-208: info keys game_id / player_id / valid_actions_mask / turn), `step(action) -> (obs, reward, terminated,
    truncated, info)` (:210-289: an action the mask rejects returns (obs, -0.1, False, False, {"invalid_action": True}) and
    the game does not advance; otherwise info carries turn / valid_actions_mask / game_status / winner), `render`, `close` -
    served by a ONE-board GeneralsVecEnv instead of a gRPC server (`server_address` is kept as an attribute only).  One board
    per launch wastes the GPU: use GeneralsVecEnv / ParallelVecEnvPool for throughput; this class is for code that wants the
    reference's object.  Opponent: the on-device random agent (the reference's default is a random opponent too, :443-497),
    or `opponent_agent` - any object with the reference's `select_action(game_state_proto) -> Action proto | None`
    (:244-255): it is handed the learner's proto GameState (wire.game_state: the reference passes `self.current_state`), its
    move is played for player 1 (GeneralsVecEnv.step(..., other_actions=...); the remaining seats of a game with more than
    two players then do not move).  `self_play` is an attribute the reference stores and never reads; so here."""
    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}

    def __init__(self, server_address="localhost:50051", board_width=15, board_height=15, max_players=2, fog_of_war=True,
                 render_mode=None, self_play=False, opponent_agent=None, max_turns=500, turn_time_ms=500,
                 collect_experiences=False, device=0, seed=0):
        self.server_address, self.board_width, self.board_height = server_address, board_width, board_height
        self.board_size = board_width * board_height
        self.max_players, self.fog_of_war, self.render_mode = max_players, fog_of_war, render_mode
        self.self_play, self.opponent_agent, self.max_turns = self_play, opponent_agent, max_turns
        self.turn_time_ms, self.collect_experiences, self.device = turn_time_ms, collect_experiences, device
        self._vec = GeneralsVecEnv(1, board_width, board_height, max_players, fog_of_war=fog_of_war, max_turns=max_turns, seed=seed,
                                   device=device, board_pool=4)
        self._seed, self._games = seed, 0
        self.game_id = None
        self.player_id = None
        self.turn_count = 0
        self.observation_space = _Box(0.0, 1.0, (9, board_height, board_width), np.float32)
        self.action_space = _Discrete(self.board_size * 5, seed)
        self.valid_actions_mask = None
        self._obs = None

    def reset(self, seed=None, options=None):
        if seed is not None:
            self._seed = seed
        self._games += 1
        obs, info = self._vec.reset(seed=self._seed * 7919 + self._games)      # a new game (CreateGame + JoinGame x2, :158-186)
        self.game_id, self.player_id, self.turn_count = f"vec-game-{self._games}", 0, 0
        self._obs = obs[0].copy()
        self.valid_actions_mask = info["valid_actions_mask"][0].copy()
        return self._obs, {"game_id": self.game_id, "player_id": self.player_id, "valid_actions_mask": self.valid_actions_mask,
                           "turn": self.turn_count}

    def _proto_state(self):
        """`self.current_state` of the reference (:256-262): the proto GameState the server sends for the learner's token."""
        from . import wire
        e = self._vec.engine
        st = e.game_state(fields=wire.STATE_FIELDS)
        vis, fog = e.compute_player_visibility(self.player_id)
        return wire.game_state(st, vis, fog, e.get_legal_action_mask(0, self.player_id), 0, self.player_id, game_id=self.game_id or "",
                               names=["RL_Agent", "Opponent"] + [f"player{p}" for p in range(2, self.max_players)])

    def _opponent_moves(self):
        """generals_env.py:244-255: `opponent_agent.select_action(self.current_state)` - the reference hands the opponent the
        LEARNER's state - returns a proto Action (or None = no move), submitted with the opponent's token (player 1)."""
        from .vec_engine import ACTION_DTYPE
        others = np.zeros((1, self.max_players), ACTION_DTYPE)
        act = self.opponent_agent.select_action(self._proto_state())
        if act:
            src = getattr(act, "from")
            others[0, 1] = (src.x, src.y, act.to.x, act.to.y, 1 | (2 if getattr(act, "half", False) else 0), (0, 0, 0))   # GVEC_ACT_VALID | _HALF
        return others

    def _will_be_played(self, action):
        """Whether the learner's own submit goes through (:226-243): the mask accepts the index (:399) and, for a half move,
        the server accepts the first in-board direction the reference sends (:419-425; a mountain there is refused)."""
        a, w, h = int(action), self.board_width, self.board_height
        if not 0 <= a < self.board_size * 5 or not self.valid_actions_mask[a]:
            return False
        if a % 5 < 4:
            return True
        x, y = (a // 5) % w, (a // 5) // w
        d = next(d for d, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0))) if 0 <= x + dx < w and 0 <= y + dy < h)
        return bool(self.valid_actions_mask[(a // 5) * 5 + d])

    def step(self, action):
        others = None
        if self.opponent_agent is not None:      # the reference asks its opponent only once the learner's submit went through (:244-253)
            from .vec_engine import ACTION_DTYPE
            others = self._opponent_moves() if self._will_be_played(action) else np.zeros((1, self.max_players), ACTION_DTYPE)
        obs, reward, terminated, truncated, info = self._vec.step(np.array([int(action)], np.int64), other_actions=others)
        self._obs = obs[0].copy()
        if info["invalid_action"][0]:                                           # :226-231
            return self._obs, -0.1, False, False, {"invalid_action": True}
        if info["error"][0]:                                                    # :240-243: the server refused the move
            return self._obs, -0.1, False, False, {"error": "move rejected by the engine"}
        self.turn_count = int(info["turn"][0])
        self.valid_actions_mask = info["valid_actions_mask"][0].copy()
        term, trunc = bool(terminated[0]), bool(truncated[0])
        return self._obs, float(reward[0]), term, trunc, {
            "turn": self.turn_count, "valid_actions_mask": self.valid_actions_mask,
            "game_status": "GAME_STATUS_FINISHED" if term else "GAME_STATUS_IN_PROGRESS",      # common.proto:60-64
            "winner": int(info["winner"][0]) if term else None}

    def render(self):
        """:563-597: the learner's view as text ("human" mode only), from the proto state like the reference's."""
        if self.render_mode != "human" or self._obs is None:
            return
        tiles = self._proto_state().board.tiles
        bar = "=" * (self.board_width * 4 + 1)
        print(f"\nTurn {self.turn_count}")
        print(bar)
        for y in range(self.board_height):
            cells = []
            for x in range(self.board_width):
                tile = tiles[y * self.board_width + x]
                if not tile.visible:
                    cells.append(" ? ")
                elif tile.type == 4:                                   # TILE_TYPE_MOUNTAIN (common.proto)
                    cells.append("###")
                elif tile.owner_id == self.player_id:
                    cells.append(f" {tile.army_count:2}")
                elif tile.owner_id >= 0:
                    cells.append(f"-{tile.army_count:2}")
                else:
                    cells.append(" . ")
            print("|" + "|".join(cells) + "|")
        print(bar)

    def close(self):
        self._vec.close()
