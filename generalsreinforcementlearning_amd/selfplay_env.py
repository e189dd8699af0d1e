"""GeneralsSelfPlayVecEnv — the gym vector env with several learners per board (self-play).

GeneralsVecEnv serves one learner (player 0) per board; the reference's plan names self-play - "symmetric game setup,
experience from both perspectives" (documentation/MASTER_PLAN.md:158-172) - as the phase after the gym env.  Here every
player of a set `learners` is a GeneralsEnv client at once: each gets its own proto view (observation, valid-action
mask, reward of generals_env.py:291-387, 499-561), each plays its own Discrete(board_size * 5) action, and the players
outside the set are the on-device random agent.  One HIP launch per step (gvec_gym_step_players).

Per-learner arrays are [B, L] (learners in ascending player id): the observation [B, L, 9, H, W] reshapes to
[B * L, 9, H, W] for a shared policy without a copy.

Differences from GeneralsVecEnv: an action the mask refuses is no move for that learner - the env still
plays its turn (one policy's mistake must not freeze the other learners) - and costs -0.1 on top of the step's reward;
a learner eliminated at the start of a step is not flagged.  Finished / truncated envs are re-dealt on their next step,
as in GeneralsVecEnv.

Buffers, reset / force_reset, numpy mode and the state methods are GymVecEnvBase's (_gym_base.py), shared with
GeneralsVecEnv; this file holds the learner set, the two launches and the zero-copy slots of step().
"""
import numpy as np

from ._gym_base import GymVecEnvBase
from ._lib import check
from ._obs_batch import check_out


class GeneralsSelfPlayVecEnv(GymVecEnvBase):
    """B boards with L learners each behind the (gymnasium-style) vector API:
    reset() -> (obs [B, L, 9, H, W], info);  step(actions [B, L]) -> (obs, reward [B, L], terminated [B], truncated [B], info).
    copy_envs / save_state / restore_state (_gym_base.py): clone, save and restore env states on the device."""
    _STEP_FLAGS = ("invalid", "error", "alive")         # gvec_gym_step_players' last three outputs
    _INFO_FLAGS = (("invalid", "invalid"), ("error", "error"), ("alive", "alive"))

    def __init__(self, num_envs, board_width=15, board_height=15, max_players=2, learners=None, fog_of_war=True, max_turns=500,
                 seed=0, device=0, board_pool=1024, device_outputs=False, strategic_features=False, feature_cap=64,
                 reward_config=None):
        """learners: the player ids that are learners (None: every player); the others are the on-device random agent.
        device_outputs=True  observation / mask / reward / flags are torch tensors on the GPU; `step` takes a CUDA int64
                             tensor [B, L] of actions.  Every tensor a step returns lives in a buffer that the step AFTER
                             NEXT reuses.
        default              numpy arrays in, numpy arrays out - the same kernel, its outputs copied to pinned host
                             buffers; the observation and mask arrays a step returns likewise stay intact until the step
                             after next.
        strategic_features=True  (needs device_outputs=True) reset / step / copy_envs / restore_state add
                             info["strategic_features"], float32 [B, L, 5, H, W]: features.strategic_features of the observation
                             they return (a step's obs_out slot included), distances capped at feature_cap.  One extra
                             launch per call.
        reward_config=RewardConfig  `step`'s rewards are the reference's CalculateRewardWithConfig with these weights
                             (reward.py) for every learner, config.invalid_action on top for a refused action, instead of
                             GeneralsEnv._calculate_reward: two extra launches per step (a reward-only snapshot before it, the
                             rewards after it) on the same stream.  info["reward_terms"] (device mode): int32 [B, L, 8].
                             Everything else a step returns is unchanged.  None: today's reward, no extra launch."""
        feat_cap = self._feature_option(strategic_features, feature_cap, device_outputs)
        reward_c = self._reward_option(reward_config)
        self._require_gpu()
        ids = list(range(max_players)) if learners is None else sorted({int(p) for p in learners})
        if not ids or ids[0] < 0 or ids[-1] >= max_players:
            raise ValueError(f"learners must be a non-empty set of player ids below max_players={max_players}: {learners}")
        self.player_ids = ids
        self.num_learners = len(ids)
        self._bits = sum(1 << p for p in ids)
        super().__init__((len(ids),), feat_cap, num_envs, board_width, board_height, max_players, fog_of_war, max_turns, seed, device,
                         board_pool, device_outputs, reward_c)

    # ---- the device path ---------------------------------------------------------------------------------
    def _learner_ids(self):
        return list(self.player_ids)

    def _observe_info(self):
        self._obs_flip ^= 1
        obs, mask = self._d_obs[self._obs_flip], self._d_mask[self._obs_flip]
        e = self.engine
        # also stores the stats the first step's rewards are measured against
        check(e.L.gvec_gym_observe_players(e.h, self._bits, self._d_turn.data_ptr(), self.max_turns, obs.data_ptr(), mask.data_ptr(),
                                           self._d_reward.data_ptr(), self._d_done.data_ptr(), self._d_winner.data_ptr()),
              "gvec_gym_observe_players")
        self.valid_actions_mask = mask.view(self._t.bool)
        return obs, self._add_features(obs, {"player_ids": list(self.player_ids), "valid_actions_mask": self.valid_actions_mask,
                                             "turn": self._d_turn.clone()})

    def _slot_args(self, k, obs_out, mask_out):
        """_step_args for a step that writes its observation and mask into the caller's tensors (zero-copy slots)."""
        t, B, L = self._t, self.num_envs, self.num_learners
        check_out(obs_out, "obs_out", (t.float32,), "float32", B * L * 9 * self.board_size, self._dev)
        check_out(mask_out, "mask_out", (t.uint8, t.bool), "uint8 / bool", B * L * self.board_size * 5, self._dev)
        ptrs, _, out, info = self._step_args(k, self._obs_flip)
        obs = obs_out.view(B, L, 9, self.board_height, self.board_width)
        info = dict(info)
        info["valid_actions_mask"] = mask_out.view(t.bool).view(B, L, self.board_size * 5)
        return ptrs[:3] + (obs_out.data_ptr(), mask_out.data_ptr()) + ptrs[5:], obs, out, info

    def _step_device(self, actions, obs_out=None, mask_out=None):
        e = self.engine
        actions = self._as_actions(actions)
        k = self._step_no
        if obs_out is None and mask_out is None:
            self._obs_flip ^= 1
            ptrs, obs, out, info = self._step_args(k, self._obs_flip)
        elif obs_out is None or mask_out is None:
            raise ValueError("obs_out and mask_out go together: give both or neither")
        else:                              # the env's own observation buffers sit this step out (and keep their rotation)
            ptrs, obs, out, info = self._slot_args(k, obs_out, mask_out)
        self.last_actions = actions        # the tensor the launch reads (kept alive until the next step)
        self._step_no += 1
        self._reward_begin()
        # ONE launch: every learner's action decoded against its own view of the resident state, the other players' moves
        # from the on-device agent, the turn (or the re-deal of a `resetting` env), then every learner's observation / mask /
        # reward and the env's flags
        check(e.L.gvec_gym_step_players(e.h, self._bits, self._seed + 1000 * self._episode + 1, actions.data_ptr(), *ptrs),
              "gvec_gym_step_players")
        self._episode += 1
        self.valid_actions_mask = info["valid_actions_mask"]
        return obs, out["reward"], out["terminated"], out["truncated"], self._reward_finish(out, self._add_features(obs, dict(info)))

    # ---- gym API ------------------------------------------------------------------------------------
    def step(self, actions, obs_out=None, mask_out=None):
        """actions: [num_envs, num_learners] indices into Discrete(board_size * 5), column j for player_ids[j].
        obs_out / mask_out (device_outputs=True only, both or neither): contiguous CUDA tensors on the env's device - float32
        with the observation's numel, uint8 or bool with the mask's - that the launch writes the observation and the mask
        straight into (a slot of a rollout store: no second copy of the rows); the returned obs and
        info["valid_actions_mask"] are views of them, and they stay intact for as long as the caller leaves them alone.  A
        slot needs no alignment beyond its dtype's.  ValueError otherwise."""
        if obs_out is not None or mask_out is not None:
            if not self.device_outputs:
                raise ValueError("obs_out / mask_out need device_outputs=True")
            return self._step_device(actions, obs_out, mask_out)
        if self.device_outputs:
            return self._step_device(actions)
        return self._step_to_numpy(*self._step_device(np.asarray(actions, np.int64)))
