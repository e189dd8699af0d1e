"""GymVecEnvBase — what the two gym vector envs (GeneralsVecEnv, GeneralsSelfPlayVecEnv) are both made of, written once.

The base owns the engine and every buffer (per-learner arrays are [num_envs] + learner_shape: `()` for the one learner of
GeneralsVecEnv, `(L,)` for self-play), the cached pointer arguments of the step kernels, reset / force_reset / close, the
numpy mode, the strategic-feature option, and clone / save / restore of env states (copy_envs / save_state /
restore_state -> env_state.VecEnvState).

A subclass declares two pieces of data
  _STEP_FLAGS   the per-learner bool outputs its step kernel writes after the eleven arguments both kernels share, in the
                kernel's order; each step buffer set gets one tensor per name
  _INFO_FLAGS   (info key, flag name): how a step's info dict names them, between "valid_actions_mask" and "winner"
and owns what differs: its constructor's own options and checks, _observe_info() (one observe pass over the batch ->
(obs, info) as reset() returns them in device mode), _learner_ids() and step().
"""
import math

import numpy as np

from ._lib import GvecError
from .env_state import CONFIG_KEYS, GVEC_E_INVALID, GVEC_E_RANGE, VecEnvState
from .vec_engine import VecEngine


class GymVecEnvBase:
    _STEP_FLAGS = ()
    _INFO_FLAGS = ()

    def _require_gpu(self):
        import torch
        if not torch.cuda.is_available():
            raise GvecError(-2, f"{type(self).__name__} needs a GPU: its observations, masks and rewards come from the HIP gym kernels "
                                "(there is no host path)")
        self._t = torch

    def __init__(self, learner_shape, feat_cap, num_envs, board_width, board_height, max_players, fog_of_war, max_turns, seed, device,
                 board_pool, device_outputs, reward_c=None):
        """After _require_gpu().  feat_cap: what _feature_option returned (a subclass calls it before any other check);
        reward_c: what _reward_option returned."""
        torch = self._t
        self._reward_c, self._reward_bits = reward_c, None
        self._feat_cap, self._feat_bufs, self._feat_flip = feat_cap, None, 0
        self.num_envs = num_envs
        self.board_width, self.board_height = board_width, board_height
        self.board_size = n = board_width * board_height
        self.max_players = max_players
        self.fog_of_war = fog_of_war
        self.max_turns = max_turns
        self.single_observation_shape = (9, board_height, board_width)   # spaces.Box(0, 1, (9,H,W), float32) generals_env.py:111-116
        self.single_action_n = n * 5                                      # spaces.Discrete(board_size*5)      generals_env.py:118-120
        self._seed = seed
        self._episode = 0
        self.engine = VecEngine(num_envs, board_width, board_height, max_players, fog_of_war=fog_of_war, device=device,
                                auto_reset=True)
        self._pool, self._pool_key = board_pool, None
        self.valid_actions_mask = None
        self._obs_flip = 0
        self.device_outputs = bool(device_outputs)
        self._dev = dev = torch.device("cuda", device)
        self.engine.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        B, per = num_envs, (num_envs,) + tuple(learner_shape)              # the shape of a per-env and of a per-learner array
        self._action_shape, self._action_numel = per, math.prod(per)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self._d_obs = [z(per + (9, board_height, board_width), torch.float32) for _ in range(2)]
        self._d_mask = [z(per + (n * 5,), torch.uint8) for _ in range(2)]
        self._d_reward, self._d_done, self._d_winner = z(per, torch.float64), z(B, torch.uint8), z(B, torch.int8)
        self._d_turn = z(B, torch.int64)
        # per-step outputs rotate through three buffer sets: what step k returns is overwritten by step k + 2
        # (needs_reset: written by step k, read by step k + 1 as `resetting` and handed out as info["reset"])
        self._d_step = [{"reward": z(per, torch.float64), **{f: z(per, torch.bool) for f in self._STEP_FLAGS},
                         "winner": z(B, torch.int8), "turn": z(B, torch.int64), "terminated": z(B, torch.bool),
                         "truncated": z(B, torch.bool), "needs_reset": z(B, torch.bool)} for _ in range(3)]
        if reward_c is not None:           # reward_config: the launch's float32 rewards and the terms they are made of, per buffer set
            for b in self._d_step:
                b["reward_f32"], b["reward_terms"] = z(per, torch.float32), z(per + (8,), torch.int32)
        self._step_no = 0
        self._arg_cache = {}
        self.last_actions = None
        if not self.device_outputs:   # pinned landing buffers for the default (numpy) mode
            pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
            self._h_obs = [pin(per + (9, board_height, board_width), torch.float32) for _ in range(2)]
            self._h_mask = [pin(per + (n * 5,), torch.bool) for _ in range(2)]

    # ---- the device path ---------------------------------------------------------------------------------
    def _reset_device(self):
        self._d_turn.zero_()
        for b in self._d_step:
            b["needs_reset"].zero_()
        return self._observe_info()        # also stores the stats the first step's reward is measured against

    def _step_args(self, k, flip):
        """For step number k (mod 3) writing observation buffer `flip`: (the pointer arguments of the step kernel from
        `resetting` on, obs, the output buffer set, info).  Computed once per combination - at 4,096 envs the launch itself
        takes ~20 us and seventeen data_ptr() calls would add half of that."""
        key = (k % 3, flip)
        a = self._arg_cache.get(key)
        if a is None:
            cur, out = self._d_step[k % 3], self._d_step[(k + 1) % 3]
            obs, mask = self._d_obs[flip], self._d_mask[flip]
            ptrs = (cur["needs_reset"].data_ptr(), self._d_turn.data_ptr(), self.max_turns, obs.data_ptr(), mask.data_ptr(),
                    out["reward"].data_ptr(), out["terminated"].data_ptr(), out["truncated"].data_ptr(), out["winner"].data_ptr(),
                    out["needs_reset"].data_ptr(), out["turn"].data_ptr()) + tuple(out[f].data_ptr() for f in self._STEP_FLAGS)
            info = {"turn": out["turn"], "valid_actions_mask": mask.view(self._t.bool), **{name: out[f] for name, f in self._INFO_FLAGS},
                    "winner": out["winner"], "reset": cur["needs_reset"]}
            a = self._arg_cache[key] = (ptrs, obs, out, info)
        return a

    def _as_actions(self, actions):
        """actions as the contiguous CUDA int64 tensor a launch reads (one entry per learner); such a tensor is passed through."""
        t = self._t
        if not (isinstance(actions, t.Tensor) and actions.is_cuda and actions.dtype == t.int64 and actions.is_contiguous()
                and actions.numel() == self._action_numel):
            if isinstance(actions, np.ndarray):
                actions = t.from_numpy(np.ascontiguousarray(actions, np.int64))
            actions = t.as_tensor(actions, dtype=t.int64).to(self._dev).reshape(self._action_shape).contiguous()
        return actions

    def _to_numpy(self, obs, info):
        """The device path's outputs as numpy arrays (default mode): observation and mask land in pinned buffers that
        alternate, so the arrays returned by step k stay intact until step k + 2."""
        i = self._obs_flip
        self._h_obs[i].copy_(obs, non_blocking=True)
        self._h_mask[i].copy_(info["valid_actions_mask"], non_blocking=True)
        out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in info.items() if k != "valid_actions_mask"}
        self._t.cuda.current_stream(self._dev).synchronize()
        out["valid_actions_mask"] = self._h_mask[i].numpy()
        self.valid_actions_mask = out["valid_actions_mask"]
        return self._h_obs[i].numpy(), out

    def _step_to_numpy(self, obs, reward, terminated, truncated, info):
        """What a step returns in the default mode, from what the device path returned."""
        obs, info = self._to_numpy(obs, info)
        return obs, reward.cpu().numpy(), terminated.cpu().numpy(), truncated.cpu().numpy(), info

    # ---- info["strategic_features"] (features.py) ----------------------------------------------------------
    @staticmethod
    def _feature_option(strategic_features, feature_cap, device_outputs):
        """The cap when the option is on, else None.  Checked before anything touches a device."""
        if not strategic_features:
            return None
        from ._obs_batch import check_cap
        if not device_outputs:
            raise ValueError("strategic_features=True needs device_outputs=True: the planes are computed on the device from the "
                             "observation tensor the step wrote")
        return check_cap(feature_cap)

    def _check_uniform_boards(self, engine=None):
        """The feature kernel reads every observation as [9, board_height, board_width].  In a padded batch of unequal board
        sizes an env's planes have its own row pitch inside the padded slot: refused with ValueError (reset, restore_state)."""
        if self._feat_cap is None:
            return
        st = (engine or self.engine).game_state(fields=("width", "height"))
        if bool((st["width"] != self.board_width).any() or (st["height"] != self.board_height).any()):
            raise ValueError(f"strategic_features=True needs every board to be {self.board_width}x{self.board_height}: this is a padded "
                             "batch of unequal board sizes")

    def _add_features(self, obs, info):
        """One extra launch on the observation just written fills info["strategic_features"] ([..., 5, H, W] for obs
        [..., 9, H, W]).  Two buffers owned by the env alternate, like the observation's: what a step returns is reused by
        the step after next.  With the option off nothing is allocated or launched and info is left as it is."""
        if self._feat_cap is None:
            return info
        from .features import strategic_features
        if self._feat_bufs is None:
            shape = tuple(obs.shape[:-3]) + (5,) + tuple(obs.shape[-2:])
            self._feat_bufs = [self._t.empty(shape, dtype=self._t.float32, device=self._dev) for _ in range(2)]
        self._feat_flip ^= 1
        info["strategic_features"] = strategic_features(obs, cap=self._feat_cap, out=self._feat_bufs[self._feat_flip])
        return info

    # ---- reward_config (reward.py) ---------------------------------------------------------------------------
    @staticmethod
    def _reward_option(reward_config):
        """The gvec_reward_config of the option, or None when it is off.  Checked before anything touches a device."""
        if reward_config is None:
            return None
        from .reward import RewardConfig
        if not isinstance(reward_config, RewardConfig):
            raise ValueError(f"reward_config must be a RewardConfig or None, not {type(reward_config).__name__}")
        return reward_config.to_c()

    def _reward_begin(self):
        """Before a step's launch(es): the reward-only snapshot of the state the step starts from.  Off: nothing."""
        if self._reward_c is None:
            return
        if self._reward_bits is None:
            self._reward_bits = sum(1 << int(p) for p in self._learner_ids())
        self.engine.experience_begin(rewards_only=True)

    def _reward_finish(self, out, info):
        """After a step's launch(es), on the same stream: CalculateRewardWithConfig of every learner against the snapshot, with
        the step's own `invalid` flags; the step's float64 reward buffer is overwritten with the float32 values and
        info["reward_terms"] (device mode) is the int32 [..., 8] they are made of.  Off: nothing is launched."""
        if self._reward_c is None:
            return info
        self.engine.experience_rewards_device(self._reward_c, self._reward_bits, out["invalid"].data_ptr(), out["reward_f32"].data_ptr(),
                                              out["reward_terms"].data_ptr())
        out["reward"].copy_(out["reward_f32"])
        if self.device_outputs:
            info["reward_terms"] = out["reward_terms"]
        return info

    # ---- gym API ------------------------------------------------------------------------------------
    def reset(self, seed=None):
        if seed is not None:
            self._seed = seed
        self.engine.reset_generated(self._seed * 1000003 + 17)
        self.engine.build_board_pool(self._pool, self._seed * 7919 + 5)
        self._pool_key = (self._pool, self._seed * 7919 + 5)
        self._check_uniform_boards()
        obs, info = self._reset_device()
        return (obs, info) if self.device_outputs else self._to_numpy(obs, info)

    def force_reset(self, env_mask):
        """Ends the running episode of the marked envs: they are re-dealt in the NEXT step (GVEC_ACT_RESET_ENV semantics),
        exactly as if that step had been preceded by terminated / truncated.  How a collector cuts an episode at its own
        length limit (ParallelEnvPool.max_steps_per_episode, vector_env.py:177) without a per-env reset() call."""
        t = self._t
        if isinstance(env_mask, t.Tensor):
            m = env_mask.to(device=self._dev, dtype=t.bool)        # a CUDA mask stays on the device: no synchronisation
        else:
            m = t.as_tensor(np.asarray(env_mask, bool)).to(self._dev)
        self.needs_reset_buffer().logical_or_(m)

    def needs_reset_buffer(self):
        """The bool[num_envs] CUDA tensor the NEXT step reads as `resetting` (written by the last step: terminated |
        truncated).  A device-side collector raises entries of it to cut episodes (gvec_pool_collect)."""
        return self._d_step[self._step_no % 3]["needs_reset"]

    def close(self):
        self.engine.close()

    # ---- clone, save and restore of env states (env_state.py: what a state holds) ---------------------------
    def state_config(self):
        e = self.engine
        return {"board_width": self.board_width, "board_height": self.board_height, "max_players": self.max_players,
                "fog_of_war": bool(self.fog_of_war), "production": list(e.production),
                "normal_growth_interval": int(e.normal_growth_interval), "max_turns": int(self.max_turns),
                "learners": list(self._learner_ids()), "num_envs": self.num_envs}

    def _env_ids(self, ids):
        t = self._t
        if isinstance(ids, t.Tensor):
            return ids.to(device=self._dev, dtype=t.int64).reshape(-1)
        return t.as_tensor(np.asarray(ids, np.int64).reshape(-1)).to(self._dev)

    def _check_ids(self, ids, what):
        B = self.num_envs
        if ids.numel() and bool(((ids < 0) | (ids >= B)).any()):
            raise GvecError(GVEC_E_RANGE, f"{what}: env id out of range [0, {B})")

    def _outputs(self):
        obs, info = self._observe_info()
        return (obs, info) if self.device_outputs else self._to_numpy(obs, info)

    def _set_rows(self, dst, turn, resetting):
        """turn_count and the `resetting` flag of the envs `dst`.  Counts as one step of the buffer rotation: the flags move
        to the next step's needs_reset buffer, so what the step before last returned stays intact."""
        cur = self._d_step[self._step_no % 3]["needs_reset"]
        nxt = self._d_step[(self._step_no + 1) % 3]["needs_reset"]
        self._d_turn[dst] = turn
        if nxt is not cur:
            nxt.copy_(cur)
        nxt[dst] = resetting
        self._step_no += 1

    def copy_envs(self, dst_ids, src_ids, check=True):
        """Env dst_ids[i] continues from env src_ids[i]'s state: the engine state (gvec_copy_envs), turn_count and the
        `resetting` flag the next step reads.  Then ONE observe pass over the batch -> (obs, info) as reset() returns them
        (device or numpy mode); the other envs' observations are what they were, and their next rewards are unchanged.
        Counts as one step for the buffer rotation: what the step before last returned is overwritten.
        src_ids may repeat (fan-out); dst_ids must be distinct and disjoint from src_ids.  check=True validates that on the
        device (ids in range, distinct destinations, no env both source and destination) and raises GvecError before
        anything is copied; check=False leaves a violation undefined.  Draws keyed by env index (the on-device agent, the
        pool re-deal) stay keyed by the destination's index."""
        t = self._t
        d, s = self._env_ids(dst_ids), self._env_ids(src_ids)
        if d.numel() != s.numel():
            raise GvecError(GVEC_E_INVALID, f"copy_envs: {d.numel()} destinations for {s.numel()} sources")
        if check:
            self._check_ids(d, "copy_envs")
            self._check_ids(s, "copy_envs")
            if t.unique(d).numel() != d.numel():
                raise GvecError(GVEC_E_INVALID, "copy_envs: a destination env is named twice")
            if bool(t.isin(d, s).any()):
                raise GvecError(GVEC_E_INVALID, "copy_envs: an env is both a source and a destination")
        if d.numel():
            self.engine.copy_envs(d, s)
            self._set_rows(d, self._d_turn[s], self.needs_reset_buffer()[s])
        return self._outputs()

    def save_state(self, env_ids=None, into=None):
        """-> VecEnvState of the envs `env_ids` (None: the whole batch, with the on-device agent's stream position: a full
        restore then replays the opponents bit for bit).  into: an earlier state of as many envs taken from an env of the
        same config, whose engine and tensors are reused (no allocation)."""
        t = self._t
        full = env_ids is None
        ids = t.arange(self.num_envs, device=self._dev) if full else self._env_ids(env_ids)
        self._check_ids(ids, "save_state")
        n = ids.numel()
        cfg = self.state_config()
        if into is not None and into.num_envs == n and into.config == cfg:
            st = into
            st.env_ids.copy_(ids)
            t.index_select(self._d_turn, 0, ids, out=st.turn_count)
            t.index_select(self.needs_reset_buffer(), 0, ids, out=st.resetting)
        else:
            e = VecEngine(n, self.board_width, self.board_height, self.max_players, fog_of_war=self.fog_of_war,
                          device=self._dev.index, production=self.engine.production,
                          normal_growth_interval=self.engine.normal_growth_interval, auto_reset=True)
            e.set_stream(t.cuda.current_stream(self._dev).cuda_stream)
            st = VecEnvState(e, ids.clone(), self._d_turn[ids], self.needs_reset_buffer()[ids], None, None, cfg)
        st.engine.copy_envs(None, ids, n=n, src=self.engine)
        st.stream = (int(self._seed), int(self._episode)) if full else None
        st.pool = self._pool_key
        return st

    def restore_state(self, state, env_ids=None):
        """The inverse of save_state: env env_ids[i] (None: the envs the state was taken from) gets the state's i-th env.
        Then one observe pass -> (obs, info) as reset() returns them; counts as one step for the buffer rotation.  A state of
        the whole batch restored with env_ids=None also restores the on-device agent's stream position (and the re-deal
        pool, when the env's differs); a partial restore leaves both where they are, so the opponents' draws continue the
        running stream.  A state taken under another config is refused with GvecError(GVEC_E_INVALID)."""
        cfg = self.state_config()
        diff = [k for k in CONFIG_KEYS if state.config.get(k) != cfg[k]]
        if diff:
            raise GvecError(GVEC_E_INVALID, f"restore_state: the state was taken under another {', '.join(diff)}")
        full = env_ids is None and state.stream is not None and state.num_envs == self.num_envs
        ids = state.env_ids if env_ids is None else self._env_ids(env_ids)
        if ids.numel() != state.num_envs:
            raise GvecError(GVEC_E_INVALID, f"restore_state: {ids.numel()} env ids for a state of {state.num_envs} envs")
        self._check_ids(ids, "restore_state")
        self._check_uniform_boards(state.engine)
        self.engine.copy_envs(ids, None, n=state.num_envs, src=state.engine)
        self._set_rows(ids, state.turn_count, state.resetting)
        if full:
            self._seed, self._episode = state.stream
            if state.pool is not None and self._pool_key != state.pool:
                self.engine.build_board_pool(*state.pool)
                self._pool_key = state.pool
        return self._outputs()
