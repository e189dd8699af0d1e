"""Clone, save and restore of gym env states on the device (gvec_copy_envs).

Both vector envs (GeneralsVecEnv, GeneralsSelfPlayVecEnv) have three methods from their base class (_gym_base.py):

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

This module holds the state object and its file format; the methods live with the buffers they move.
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
