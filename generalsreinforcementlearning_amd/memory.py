"""ObservationMemory — what a learner last saw of every tile, carried from observation to observation: four planes per view
(seen, last owner, last army, age; include/generals_vec.h "fog-of-war memory planes").

Under fog of war an observation shows owner and army of the tiles visible this turn only: an enemy general seen ten turns ago
is, today, a general tile owned by nobody with army 0.  The memory is the state that outlives one observation, for learners
without recurrent state of their own.

    mem = ObservationMemory((env.num_envs, env.num_learners), H, W)
    obs, info = env.reset()
    planes = mem.update(obs)                              # [B, L, 4, H, W]
    obs, reward, terminated, truncated, info = env.step(actions)
    planes = mem.update(obs, info["reset"])               # a re-dealt env's rows start blank again
    x = torch.cat([obs, planes], dim=-3)                  # a 13-channel torso input
    feats = strategic_features(remembered_observation(obs, planes))   # distances to the enemies seen so far

One HIP launch per update (gvec_obs_memory_update: lane = tile, every byte moved once) on the current torch stream; nothing
synchronises with the host.  SelfPlayRolloutBuffer(env, horizon, memory=mem) keeps the planes of every step next to the
observations.
"""
import ctypes as C

from . import _obs_batch as ob
from ._lib import ObsMemoryArgs, check, load

NUM_MEMORY_PLANES = 4
MEMORY_PLANE_NAMES = ("seen", "last_owner", "last_army", "age")


def remembered_observation(obs, memory):
    """obs [..., 9, H, W] and its memory planes [..., 4, H, W] -> the nine-plane observation whose owner and army planes
    are the remembered ones: cat(obs[0:1], memory[1:3], obs[3:9]).  On visible tiles the memory holds the observation's own
    values and on the others the observation holds zeros, so nothing shown is lost.  strategic_features of it measures the
    distance to the nearest enemy tile seen so far and the front line against remembered enemies.  Plain torch."""
    import torch
    if obs.shape[-3] != 9 or memory.shape[-3] != NUM_MEMORY_PLANES or obs.shape[:-3] + obs.shape[-2:] != memory.shape[:-3] + memory.shape[-2:]:
        raise ValueError(f"obs {tuple(obs.shape)} and memory {tuple(memory.shape)} are not [..., 9, H, W] and [..., 4, H, W] of the same rows")
    return torch.cat([obs[..., 0:1, :, :], memory[..., 1:3, :, :], obs[..., 3:9, :, :]], dim=-3)


class ObservationMemory:
    def __init__(self, rows_shape, height, width, cap=64, device=None):
        """rows_shape: the leading dimensions of the observations, e.g. (num_envs, num_learners) (an int n means (n,)).
        cap: a power of two in [2, 1024]; age is min(updates since last visible, cap) / cap.  device: a CUDA device (None:
        the first observation's).  Nothing is allocated until the planes are read or updated."""
        import torch
        self._t = torch
        self.cap = ob.check_cap(cap)
        if isinstance(rows_shape, int) and not isinstance(rows_shape, bool):
            rows_shape = (rows_shape,)
        if not all(isinstance(n, int) and not isinstance(n, bool) and n >= 0 for n in rows_shape):
            raise ValueError(f"rows_shape {rows_shape!r} must be a tuple of ints >= 0")
        self.rows_shape = tuple(rows_shape)
        self.height, self.width = H, W = int(height), int(width)
        ob.check_board(W, H)
        self.rows = 1
        for n in self.rows_shape:
            self.rows *= n
        if self.rows >= 2 ** 31:
            raise ValueError(f"rows_shape {self.rows_shape} holds {self.rows} rows: at most 2^31 - 1")
        self.shape = self.rows_shape + (NUM_MEMORY_PLANES, H, W)
        self._dev = None if device is None else torch.device(device)
        if self._dev is not None and self._dev.type != "cuda":
            raise ValueError(f"device {self._dev} is not a CUDA device: the planes are updated by a HIP kernel (there is no host path)")
        self._planes = None          # None: blank, and not materialised yet

    # ---- state --------------------------------------------------------------------------------------------------------
    def _device(self):
        if self._dev is None or self._dev.index is None:
            self._dev = self._t.device("cuda", self._t.cuda.current_device())
        return self._dev

    def _blank(self):
        p = self._t.zeros(self.shape, dtype=self._t.float32, device=self._device())
        p[..., 3, :, :] = 1.0
        return p

    @property
    def planes(self):
        """The current state, float32 rows_shape + (4, H, W): blank after construction and reset_all(), afterwards wherever
        the last update wrote it."""
        if self._planes is None:
            self._planes = self._blank()
        return self._planes

    def reset_all(self):
        """Every row starts blank again (seen 0, owner 0, army 0, age 1.0).  The next update writes all of it."""
        self._planes = None

    def move_to(self, out):
        """Copies the state into `out` (as update's out=) and continues from there."""
        out = self._check_out(out, self.planes.device)
        out.view(self.shape).copy_(self.planes)
        self._planes = out.view(self.shape)
        return self._planes

    def _check_out(self, out, dev):
        return ob.check_out(out, "out", (self._t.float32,), "float32", self.rows * NUM_MEMORY_PLANES * self.height * self.width, dev)

    # ---- the update ---------------------------------------------------------------------------------------------------
    def update(self, obs, reset=None, out=None):
        """One turn: obs CUDA float32 rows_shape + (9, H, W), read in place when its rows have one common stride (a rollout
        slot, one learner of every env) and copied otherwise.  reset: bool / uint8 CUDA tensor whose shape is a leading
        prefix of rows_shape - info["reset"] [B] for rows_shape (B, L) - a set flag restarts its rows from blank before the
        observation is applied.  out: a contiguous float32 CUDA tensor of the state's size that takes the new state (every
        element is written); `planes` is then a view of it.  None: the state is updated in place.  Returns `planes`.
        One launch on the current stream.  TypeError / ValueError before any launch."""
        t = self._t
        H, W = self.height, self.width
        # types and shapes first, devices after: a wrong shape is reported as such whatever holds the tensor
        ob.check_tensor(obs, "obs", (t.float32,))
        if tuple(obs.shape) != self.rows_shape + (9, H, W):
            raise ValueError(f"obs {tuple(obs.shape)} is not {self.rows_shape + (9, H, W)}")
        rows_per_flag = 1
        if reset is not None:
            ob.check_tensor(reset, "reset", (t.bool, t.uint8))
            k = reset.dim()
            if tuple(reset.shape) != self.rows_shape[:k]:
                raise ValueError(f"reset {tuple(reset.shape)} is no leading prefix of rows_shape {self.rows_shape}")
            for n in self.rows_shape[k:]:
                rows_per_flag *= n
        ob.check_device("the planes are updated by a HIP kernel", "obs", obs=obs)
        if self._dev is None or self._dev.index is None:
            self._dev = obs.device
        dev = self._dev
        if obs.device != dev:
            raise ValueError(f"obs is on {obs.device}, the memory on {dev}")
        if reset is not None:
            if reset.device != dev:
                raise ValueError(f"reset must be a CUDA tensor on {dev}")
            reset = reset.contiguous()
        if out is not None:
            out = self._check_out(out, dev)
        obs, stride = ob.in_place(obs, 3, H, W)
        prev = self._planes
        if out is None:
            out = prev if prev is not None else t.empty(self.shape, dtype=t.float32, device=dev)
        if self.rows:
            a = ObsMemoryArgs(rows=self.rows, width=W, height=H, cap=self.cap, rows_per_flag=rows_per_flag, obs_row_stride=stride,
                              obs=obs.data_ptr(), prev=ob.ptr(prev), reset=ob.ptr(reset), out=out.data_ptr())
            check(load().gvec_obs_memory_update(dev.index, ob.stream(dev), C.byref(a)), "gvec_obs_memory_update")
        self._planes = out.view(self.shape)
        return self._planes

    # ---- beside env.copy_envs / save_state ------------------------------------------------------------------------------
    def copy_envs(self, dst_ids, src_ids):
        """Mirrors env.copy_envs(dst_ids, src_ids): the rows of env dst_ids[i] (the first dimension of rows_shape) continue
        from those of env src_ids[i].  Torch indexing, no update: the observation after a copy is not a new turn."""
        t = self._t
        p = self.planes
        d = t.as_tensor(dst_ids, dtype=t.int64, device=p.device).reshape(-1)
        s = t.as_tensor(src_ids, dtype=t.int64, device=p.device).reshape(-1)
        if d.numel() != s.numel():
            raise ValueError(f"copy_envs: {d.numel()} destinations for {s.numel()} sources")
        if d.numel():
            p[d] = p[s]

    def state_dict(self):
        """A copy of the state with what it was built for; goes beside env.save_state()."""
        return {"planes": self.planes.clone(), "cap": self.cap, "rows_shape": self.rows_shape, "height": self.height, "width": self.width}

    def load_state_dict(self, state):
        for k in ("cap", "rows_shape", "height", "width"):
            if (tuple(state[k]) if k == "rows_shape" else state[k]) != getattr(self, k):
                raise ValueError(f"load_state_dict: the state was saved with {k} = {state[k]}, this memory has {getattr(self, k)}")
        src = state["planes"]
        if tuple(src.shape) != self.shape or src.dtype != self._t.float32:
            raise ValueError(f"load_state_dict: planes {tuple(src.shape)} {src.dtype} are not float32 {self.shape}")
        self.planes.copy_(src)
