"""Clone, save and restore of gym env states on the device (gvec_copy_envs).

Both vector envs (GeneralsVecEnv, GeneralsSelfPlayVecEnv) get three methods from `EnvStateMixin`:

  copy_envs(dst_ids, src_ids)        in-batch cloning: env dst_ids[i] continues from env src_ids[i]'s state - the fan-out
                                     of a tree search ("copy root r into children c1..ck, step each child differently")
  save_state(env_ids=None, into=None) -> VecEnvState: the named envs copied into a private engine of their own
  restore_state(state, env_ids=None) the inverse: rewind a batch and replay it exactly

and `VecEnvState.save(path)` / `VecEnvState.load(path)` put a state in one .npz file on top of the canonical record slab
(gvec_export_records / gvec_import_records, which validates every header on the device).

What a state holds per env: the engine state (header, planes, armies), the gym `turn_count` and the `resetting` flag the
next step reads (the env is re-dealt in that step).  The reward baseline is not part of it: after any gym call every env's
stored player stats equal its current ones, and the methods here end with one observe pass over the batch, which stores
them again - for the envs that were not copied too, where it changes nothing.
"""
import json

import numpy as np

from ._lib import GvecError
from .vec_engine import VecEngine

GVEC_E_INVALID, GVEC_E_RANGE = -1, -4
FORMAT_VERSION = 1
# what must agree between the env a state was taken from and the env it is restored into
CONFIG_KEYS = ("board_width", "board_height", "max_players", "fog_of_war", "production", "normal_growth_interval", "max_turns",
               "learners")


class VecEnvState:
    """Snapshot of some envs of a vector env (save_state).  Fields:
    engine      a VecEngine of capacity num_envs holding the envs' engine state (env i = the i-th saved env)
    env_ids     int64 CUDA tensor [num_envs]: the env slots they were taken from (restore_state's default target)
    turn_count  int64 CUDA tensor [num_envs]
    resetting   bool CUDA tensor [num_envs]: the env is re-dealt by the next step
    stream      (seed, episode) of the on-device agent's stream when the whole batch was saved, else None
    pool        (board_pool, pool seed) the batch's re-deal pool was built with
    config      dict of CONFIG_KEYS (+ num_envs of the batch it came from)"""

    def __init__(self, engine, env_ids, turn_count, resetting, stream, pool, config):
        self.engine, self.env_ids, self.turn_count, self.resetting = engine, env_ids, turn_count, resetting
        self.stream, self.pool, self.config = stream, pool, config

    @property
    def num_envs(self):
        return self.engine.B

    def save(self, path):
        """Writes one .npz: the canonical record slab of the envs, turn_count, resetting, the stream position, the pool
        and the config."""
        import torch
        e = self.engine
        dev = torch.device("cuda", e.device)
        slab = torch.empty(e.B * e.state_bytes_per_env(), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            e.export_records(slab.data_ptr())
            records = slab.cpu().numpy()      # synchronises the stream the engine works on (the env's)
        meta = {"version": FORMAT_VERSION, "config": self.config, "stream": self.stream, "pool": self.pool}
        with open(path, "wb") as f:
            np.savez(f, records=records, turn_count=self.turn_count.cpu().numpy(), resetting=self.resetting.cpu().numpy(),
                     env_ids=self.env_ids.cpu().numpy(), meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path, device=0):
        """Reads a state written by save().  Every record header is validated on the device (gvec_import_records:
        GvecError GVEC_E_BOARD on a record that does not fit the config)."""
        import torch
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            records, turn, resetting, ids = z["records"], z["turn_count"], z["resetting"], z["env_ids"]
        if meta.get("version") != FORMAT_VERSION:
            raise GvecError(GVEC_E_INVALID, f"{path}: env state format {meta.get('version')}, this build reads {FORMAT_VERSION}")
        c = meta["config"]
        n = len(turn)
        dev = torch.device("cuda", device)
        e = VecEngine(n, c["board_width"], c["board_height"], c["max_players"], fog_of_war=c["fog_of_war"], device=device,
                      production=tuple(c["production"]), normal_growth_interval=c["normal_growth_interval"], auto_reset=True)
        e.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        if records.size != n * e.state_bytes_per_env():
            raise GvecError(GVEC_E_INVALID, f"{path}: {records.size} record bytes for {n} envs of {e.state_bytes_per_env()} bytes")
        slab = torch.from_numpy(records).to(dev)
        e.import_records(slab.data_ptr())
        as_t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        stream = None if meta["stream"] is None else tuple(int(v) for v in meta["stream"])
        pool = None if meta["pool"] is None else tuple(int(v) for v in meta["pool"])
        return cls(e, as_t(ids, torch.int64), as_t(turn, torch.int64), as_t(resetting, torch.bool), stream, pool, c)


class EnvStateMixin:
    """copy_envs / save_state / restore_state for the vector envs.  The env provides engine, num_envs, _t, _dev, _d_turn,
    _d_step, _step_no, _seed, _episode, _pool, device_outputs, _to_numpy, _observe_info() (one observe pass over the batch
    -> (obs, info) as reset() returns them in device mode), _learner_ids() and _feat_cap / _feat_bufs / _feat_flip
    (_feature_option, _add_features)."""

    def state_config(self):
        e = self.engine
        return {"board_width": self.board_width, "board_height": self.board_height, "max_players": self.max_players,
                "fog_of_war": bool(self.fog_of_war), "production": list(e.production),
                "normal_growth_interval": int(e.normal_growth_interval), "max_turns": int(self.max_turns),
                "learners": list(self._learner_ids()), "num_envs": self.num_envs}

    # ---- info["strategic_features"] (features.py): the option of both envs ----
    @staticmethod
    def _feature_option(strategic_features, feature_cap, device_outputs):
        """The cap when the option is on, else None.  Checked before anything touches a device."""
        if not strategic_features:
            return None
        from .features import check_cap
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
        st.pool = getattr(self, "_pool_key", None)
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
            if state.pool is not None and getattr(self, "_pool_key", None) != state.pool:
                self.engine.build_board_pool(*state.pool)
                self._pool_key = state.pool
        return self._outputs()
