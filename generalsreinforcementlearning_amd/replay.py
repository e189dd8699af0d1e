"""The replay memories: `ReplayBuffer` on the host, `DeviceReplayBuffer` and `PrioritizedDeviceReplayBuffer` in HBM.

Reference: python/generals_gym/replay_buffer.py:13-55 (a thread-safe ring of (state, action, reward, next_state, done)).
`ReplayBuffer` is that class over arrays.  The two device rings keep its semantics for a pool that never leaves the GPU
(env_pool.ParallelVecEnvPool): a collector hands a ring each vector step through `append_step`, and the ring itself makes
the launches that append the rows and keep what rides beside them - the n-step links and the priority tree
 - in the one order both rest on.

Locking, the same rule in all three: every method that reads or writes the ring takes `_guard`, a plain Lock, once; a
method with a leading underscore that touches the ring expects its caller to hold it.  Nothing takes it twice: a public
method never calls another public method that locks (`PrioritizedDeviceReplayBuffer.push_batch` goes through `_rows` /
`_write_rows`, `sample_nstep` through `_sample_indices`).
"""
import ctypes
import random
import threading

import numpy as np

from ._lib import PER_HDR_DRAWS, PER_HDR_REJECTED, PER_HEADER_WORDS, NstepGatherArgs, check, load
from ._sampling import distinct_indices


class ReplayBuffer:
    """Thread-safe ring-buffer replay memory (replay_buffer.py:13-55): `push` evicts the oldest transition when full,
    `sample` draws uniformly without replacement with the module-level `random` (same indices as the reference's
    `random.sample(list, k)` for the same seed: the draw depends on the length only), `total_pushed` is the monotonic
    env-step counter, `len()` the fill.  Stored as arrays (one slab per field, allocated at the first push) rather than a
    list of tuples, so `push_batch` writes a whole vector step under one lock and `sample_arrays` hands a learner stacked
    batches without a Python loop."""

    copies_what_it_is_given = True      # push / push_batch keep no reference to their arguments: a pool may hand over the env's own arrays

    def __init__(self, capacity):
        if capacity <= 0:
            raise ValueError(f"capacity must be positive, got {capacity}")   # replay_buffer.py:22-23
        self.capacity = int(capacity)
        self._state = self._next = self._action = self._reward = self._done = None
        self._size = 0          # transitions held
        self._cursor = 0        # slot the next transition goes to
        self._pushed = 0        # every push since construction
        self._guard = threading.Lock()

    def _alloc(self, state):
        s = np.asarray(state)
        self._state = np.empty((self.capacity,) + s.shape, s.dtype)
        self._next = np.empty((self.capacity,) + s.shape, s.dtype)
        self._action = np.empty(self.capacity, np.int64)
        self._reward = np.empty(self.capacity, np.float64)
        self._done = np.empty(self.capacity, bool)

    def push(self, state, action, reward, next_state, done):
        with self._guard:
            if self._state is None:
                self._alloc(state)
            slot = self._cursor
            self._state[slot], self._next[slot] = state, next_state
            self._action[slot], self._reward[slot], self._done[slot] = action, reward, done
            self._cursor = (slot + 1) % self.capacity                       # the oldest slot is the next to go (:31-36)
            self._size = min(self._size + 1, self.capacity)
            self._pushed += 1

    def push_batch(self, states, actions, rewards, next_states, dones):
        """k transitions in order (equivalent to k `push` calls) under one lock."""
        k = len(actions)
        if k == 0:
            return
        with self._guard:
            if self._state is None:
                self._alloc(states[0])
            first = self._cursor
            if k > self.capacity:                                            # only the last `capacity` survive, as with k pushes
                keep = slice(k - self.capacity, k)
                first = (first + k - self.capacity) % self.capacity
                states, actions, rewards, next_states, dones = states[keep], actions[keep], rewards[keep], next_states[keep], dones[keep]
            n = len(actions)
            head = min(n, self.capacity - first)                             # two contiguous runs (the ring wraps at most once): memcpy, not a gather
            for dst, src in ((self._state, states), (self._next, next_states), (self._action, actions), (self._reward, rewards), (self._done, dones)):
                dst[first:first + head] = src[:head]
                if head < n:
                    dst[:n - head] = src[head:]
            self._cursor = (self._cursor + k) % self.capacity
            self._size = min(self._size + k, self.capacity)
            self._pushed += k

    def _item(self, i):
        return (self._state[i], int(self._action[i]), float(self._reward[i]), self._next[i], bool(self._done[i]))

    def sample(self, batch_size):
        """List of (state, action, reward, next_state, done) tuples, like the reference (:40-43); ValueError when the
        buffer holds fewer than batch_size transitions (random.sample's own)."""
        with self._guard:
            return [self._item(i) for i in random.sample(range(self._size), batch_size)]

    def sample_arrays(self, batch_size):
        """The same draw as stacked arrays: (states, actions, rewards, next_states, dones)."""
        with self._guard:
            idx = np.asarray(random.sample(range(self._size), batch_size), np.int64)
            return self._state[idx], self._action[idx], self._reward[idx], self._next[idx], self._done[idx]

    @property
    def total_pushed(self):
        with self._guard:
            return self._pushed

    def __len__(self):
        with self._guard:
            return self._size


class DeviceReplayBuffer:
    """The replay ring resident in HBM: what `ReplayBuffer` is to a host collector, for a pool that never leaves the GPU
    (`ParallelVecEnvPool` over a `GeneralsVecEnv(device_outputs=True)`).  Transitions are appended by `gvec_pool_collect`
    (one wavefront moves one row) straight from the gym kernel's output buffers; `sample_arrays` gathers a batch into CUDA
    tensors a learner consumes in place.  288 GB of HBM hold 17 million 15x15 transitions (2 x 8,100 B of observation each).
    Same semantics as replay_buffer.py:13-55 - the oldest transition is overwritten once `capacity` is reached, `sample`
    draws uniformly without replacement and raises ValueError when fewer than batch_size are held, `total_pushed` counts
    every push - with one difference: the draw comes from a torch generator on the device, not from `random`.

    `n_step` > 1 adds multi-step returns: the ring then keeps `ring_succ`, one int64 link per slot to the
    same worker's next transition of the same episode (written on the device by gvec_nstep_link right after
    gvec_pool_collect, in `append_step`; -1 where the episode ended, was cut, or the row came from `push_batch`), and
    `sample_nstep` / `gather_nstep` return `(states, actions, returns, next_states, dones, discounts, steps)` from ONE fused
    gather (gvec_nstep_gather): `returns` the discounted sum of up to n_step rewards, `next_states` / `dones` those of the
    last row of the chain, `discounts = gamma ** steps` - a learner's target is `returns + discounts * (1 - dones) * max Q(next)`.
    They work on an n_step == 1 buffer too (returns == rewards, discounts == gamma), which allocates nothing more.
    `sample_arrays` / `sample` stay one-step whatever n_step is: a learner written for them bootstraps with gamma."""

    _keeps_tree = False                          # the prioritized class: rows that arrive need leaves (gvec_per_push)

    def __init__(self, capacity, device=0, n_step=1, gamma=0.99):
        if capacity <= 0:
            raise ValueError(f"capacity must be positive, got {capacity}")
        if int(n_step) != n_step or n_step < 1 or not 0.0 <= float(gamma) < float("inf"):
            raise ValueError(f"n_step {n_step} must be an integer >= 1 and gamma {gamma} finite and >= 0")
        import torch
        self._t, self._L = torch, load()
        self.capacity = int(capacity)
        self.device = torch.device("cuda", device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=self.device)     # cursor, size, total pushed, 0
        self.state = self.next_state = self.action = self.reward = self.done = None
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(0)
        self._guard = threading.Lock()            # the module docstring has the rule that keeps it from being taken twice
        self.n_step, self.gamma = int(n_step), float(gamma)
        self.ring_succ = None                     # int64 [capacity] once allocated, and only when n_step > 1
        # the counters ahead of an append, for the kernels that learn from them on the device how many rows came and where:
        # gvec_nstep_link (n_step > 1) and gvec_per_push (a priority tree); one 32-byte copy serves both
        self._before = torch.zeros(4, dtype=torch.int64, device=self.device) if self.n_step > 1 or self._keeps_tree else None

    def allocate(self, obs_shape):
        """The five slabs of the ring (at the first push; a collector calls it with the env's observation shape), and the
        successor links of an n_step > 1 buffer."""
        if self.n_step > 1 and self.ring_succ is None:
            self.ring_succ = self._t.full((self.capacity,), -1, dtype=self._t.int64, device=self.device)
        if self.state is None:
            t, dev, cap = self._t, self.device, self.capacity
            self.obs_shape = tuple(obs_shape)
            self.state = t.empty((cap,) + self.obs_shape, dtype=t.float32, device=dev)
            self.next_state = t.empty((cap,) + self.obs_shape, dtype=t.float32, device=dev)
            self.action = t.empty(cap, dtype=t.int64, device=dev)
            self.reward = t.empty(cap, dtype=t.float64, device=dev)
            self.done = t.empty(cap, dtype=t.bool, device=dev)
        return self

    def ring_pointers(self):
        """(field, tensor) of the six ring_* pointers gvec_collect_args and gvec_nstep_gather_args share; the ring is allocated."""
        return (("ring_state", self.state), ("ring_next_state", self.next_state), ("ring_action", self.action),
                ("ring_reward", self.reward), ("ring_done", self.done), ("ring_counters", self.counters))

    def _stream(self):
        return self._t.cuda.current_stream(self.device).cuda_stream

    def manual_seed(self, seed):
        self._gen.manual_seed(int(seed))

    def append_step(self, args, stream, nstep_last):
        """A collector's vector step arrives: `args` is its gvec_collect_args (the ring's own fields filled from
        `ring_pointers`), `nstep_last` its per-worker link state (None when n_step == 1).  The order - copy the counters,
        append, link, leaves - is what the links and the tree rest on, and the guard orders all of it against a learner's
        sample_arrays / push_batch on the same stream."""
        dev = self.device.index
        with self._guard:
            if self._before is not None:
                self._before.copy_(self.counters)
            check(self._L.gvec_pool_collect(dev, stream, ctypes.byref(args)), "gvec_pool_collect")
            if self.n_step > 1:
                check(self._L.gvec_nstep_link(dev, stream, ctypes.byref(args), self._before.data_ptr(), self.ring_succ.data_ptr(),
                                              nstep_last.data_ptr()), "gvec_nstep_link")
            self._rows_appended(args.num_envs, stream)

    def _rows_appended(self, max_count, stream):
        """Up to `max_count` rows came since the counters were copied to `_before`; the caller holds `_guard`."""

    def _rows(self, states, actions, rewards, next_states, dones):
        """push_batch's arguments with states and actions as device tensors (rewards and dones are converted where they are
        written); None when there are no rows."""
        t, dev = self._t, self.device
        actions = t.as_tensor(actions, dtype=t.int64, device=dev).reshape(-1)
        if actions.numel() == 0:
            return None
        return t.as_tensor(states, dtype=t.float32, device=dev), actions, rewards, t.as_tensor(next_states, dtype=t.float32, device=dev), dones

    def _write_rows(self, states, actions, rewards, next_states, dones):
        """`_rows` into the ring, in order; the caller holds `_guard`."""
        t, dev, k = self._t, self.device, int(actions.numel())
        self.allocate(states.shape[1:])
        cursor, size, pushed = (int(v) for v in self.counters[:3].tolist())
        lo = max(0, k - self.capacity)                                    # only the last `capacity` survive, as with k pushes
        idx = (cursor + t.arange(lo, k, device=dev)) % self.capacity
        self.state[idx], self.next_state[idx] = states[lo:], next_states[lo:]
        self.action[idx] = actions[lo:]
        self.reward[idx] = t.as_tensor(rewards, dtype=t.float64, device=dev).reshape(-1)[lo:]
        self.done[idx] = t.as_tensor(dones, dtype=t.bool, device=dev).reshape(-1)[lo:]
        if self.ring_succ is not None:
            self.ring_succ[idx] = -1                                      # no worker, no episode: such a row is a chain of one
        self.counters[:3] = t.tensor([(cursor + k) % self.capacity, min(size + k, self.capacity), pushed + k], dtype=t.int64)

    def push_batch(self, states, actions, rewards, next_states, dones):
        """k transitions in order, for a learner that pushes by itself (the pool appends through `append_step`)."""
        rows = self._rows(states, actions, rewards, next_states, dones)
        if rows is not None:
            with self._guard:
                self._write_rows(*rows)

    def push(self, state, action, reward, next_state, done):
        t = self._t
        self.push_batch(t.as_tensor(state)[None], [action], [reward], t.as_tensor(next_state)[None], [done])

    def _sample_indices(self, batch_size):
        """The draw of `sample_indices` for a caller inside the class, which holds `_guard`."""
        return distinct_indices(self._t, len(self), batch_size, self.device, self._gen)

    def sample_indices(self, batch_size):
        """batch_size distinct slots, uniformly over the transitions held (random.sample's contract, replay_buffer.py:40-43)."""
        return self._sample_indices(batch_size)

    def sample_arrays(self, batch_size):
        """(states, actions, rewards, next_states, dones) as CUDA tensors.  The draw and its five gathers are enqueued under
        the lock a collector's launches take too, so no vector step lands between them: a drawn slot's fields belong to ONE
        transition even while the ring is being overwritten (the reference samples under its lock as well, :40-43)."""
        with self._guard:
            idx = self._sample_indices(batch_size)
            return self.state[idx], self.action[idx], self.reward[idx], self.next_state[idx], self.done[idx]

    def sample(self, batch_size):
        """The reference's return type - a list of (state, action, reward, next_state, done) tuples - on the host."""
        s, a, r, n, d = (x.cpu().numpy() for x in self.sample_arrays(batch_size))
        return [(s[i], int(a[i]), float(r[i]), n[i], bool(d[i])) for i in range(len(a))]

    def _gather_nstep(self, idx):
        """One launch of gvec_nstep_gather over `idx`; the caller holds `_guard`."""
        t, dev = self._t, self.device
        if self.state is None:
            raise ValueError("the replay buffer is empty")
        idx = t.as_tensor(idx, device=dev).to(t.int64).reshape(-1).contiguous()
        k = int(idx.numel())
        a = NstepGatherArgs()
        a.k, a.capacity, a.n_step, a.obs_floats, a.gamma = k, self.capacity, self.n_step, int(np.prod(self.obs_shape)), self.gamma
        out = dict(state=t.empty((k,) + self.obs_shape, dtype=t.float32, device=dev), next_state=t.empty((k,) + self.obs_shape, dtype=t.float32, device=dev),
                   action=t.empty(k, dtype=t.int64, device=dev), ret=t.empty(k, dtype=t.float64, device=dev),
                   discount=t.empty(k, dtype=t.float64, device=dev), done=t.empty(k, dtype=t.bool, device=dev),
                   steps=t.empty(k, dtype=t.int32, device=dev), last_idx=t.empty(k, dtype=t.int64, device=dev))
        for name, tensor in (("idx", idx),) + self.ring_pointers() + tuple(out.items()):
            setattr(a, name, tensor.data_ptr())
        a.ring_succ = None if self.ring_succ is None else self.ring_succ.data_ptr()
        check(self._L.gvec_nstep_gather(dev.index, self._stream(), ctypes.byref(a)), "gvec_nstep_gather")
        return out

    @staticmethod
    def _seven(o):
        return o["state"], o["action"], o["ret"], o["next_state"], o["done"], o["discount"], o["steps"]

    def gather_nstep(self, idx):
        """(states, actions, returns, next_states, dones, discounts, steps) for the slots `idx`: per slot the chain of up to
        n_step transitions of one worker's episode that starts there.  A slot outside [0, len) gives steps 0, returns 0,
        discounts 0, action -1 and zero rows."""
        with self._guard:
            return self._seven(self._gather_nstep(idx))

    def sample_nstep(self, batch_size):
        """The buffer's own draw (`sample_indices`) and its n-step gather, enqueued under the lock a collector's launches take
        too, like `sample_arrays`: no vector step lands between the draw and the walk."""
        with self._guard:
            return self._seven(self._gather_nstep(self._sample_indices(batch_size)))

    @property
    def total_pushed(self):
        return int(self.counters[2])

    def __len__(self):
        return int(self.counters[1])


class PrioritizedDeviceReplayBuffer(DeviceReplayBuffer):
    """`DeviceReplayBuffer` with prioritized experience replay (Schaul et al. 2016) on the device: a radix-64 float32 sum tree
    over the ring's slots, kept and sampled by the gvec_per_* kernels.  A slot's priority is
    `(|td_error| + eps) ** alpha`; a new transition - pushed here or appended by the pool's `gvec_pool_collect` - gets the
    largest priority ever written (1.0 at the start); a slot that holds no transition has priority 0 and is never drawn.
    `sample_prioritized` makes `batch_size` stratified draws WITH replacement and returns the importance weights
    `(len * P(i)) ** -beta` over the batch's largest; `sample_arrays` / `sample` are that draw without indices and weights, so
    a learner or pool written for the uniform buffer runs unchanged.  `update_priorities(indices, td_errors)` takes the
    indices of an earlier draw: a slot the collector has overwritten in between simply takes the stale priority, as in
    standard prioritized replay (there is no generation check).  Nothing here synchronises except `len()`."""

    _keeps_tree = True

    def __init__(self, capacity, device=0, alpha=0.6, beta=0.4, eps=1e-6, n_step=1, gamma=0.99):
        if alpha < 0 or beta < 0 or not eps > 0:
            raise ValueError(f"alpha {alpha} and beta {beta} must be >= 0 and eps {eps} > 0")
        super().__init__(capacity, device, n_step=n_step, gamma=gamma)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        layout = (ctypes.c_int64 * 10)()
        check(self._L.gvec_per_tree_layout(self.capacity, layout), "gvec_per_tree_layout")
        self.tree_levels, self._tree_words = int(layout[0]), int(layout[1])
        self.tree_offsets = [int(layout[2 + l]) for l in range(self.tree_levels + 1)]     # in floats; level 0 = the leaves
        self.tree = None
        self._seed = 0

    def allocate(self, obs_shape):
        super().allocate(obs_shape)
        if self.tree is None:
            t = self._t
            self.tree = t.empty(self._tree_words, dtype=t.float32, device=self.device)
            check(self._L.gvec_per_init(self.device.index, self._stream(), self.tree.data_ptr(), self.capacity), "gvec_per_init")
        return self

    def _header(self):
        return self.tree[:PER_HEADER_WORDS].view(self._t.int32)

    def manual_seed(self, seed):
        """Seeds the draw: the same seed over the same ring gives the same indices (the sequence restarts)."""
        super().manual_seed(seed)
        with self._guard:
            self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            if self.tree is not None:
                self._header()[PER_HDR_DRAWS:PER_HDR_DRAWS + 2].zero_()

    def _rows_appended(self, max_count, stream):
        """The rows get the maximum priority."""
        check(self._L.gvec_per_push(self.device.index, stream, self.tree.data_ptr(), self.capacity, self._before.data_ptr(),
                                    self.counters.data_ptr(), int(max_count)), "gvec_per_push")

    def push_batch(self, states, actions, rewards, next_states, dones):
        k = int(self._t.as_tensor(actions).numel())
        if k == 0:
            return
        with self._guard:                        # one acquisition: no collector step or update lands between the rows and their leaves
            self._before.copy_(self.counters)
            self._write_rows(*self._rows(states, actions, rewards, next_states, dones))
            self._rows_appended(min(k, self.capacity), self._stream())

    def update_priorities(self, indices, td_errors):
        """priority[indices[i]] = (|td_errors[i]| + eps) ** alpha; duplicates: one of the values wins; an index outside the
        ring or a non-finite error is skipped on the device and counted in `rejected_updates`."""
        t = self._t
        idx = t.as_tensor(indices, device=self.device).to(t.int64).reshape(-1).contiguous()
        td = t.as_tensor(td_errors, device=self.device).detach().to(t.float32).reshape(-1).contiguous()
        if idx.numel() != td.numel():
            raise ValueError(f"{idx.numel()} indices, {td.numel()} td errors")
        if idx.numel() == 0 or self.tree is None:
            return
        with self._guard:
            check(self._L.gvec_per_update(self.device.index, self._stream(), self.tree.data_ptr(), self.capacity, idx.data_ptr(),
                                          td.data_ptr(), idx.numel(), self.alpha, self.eps), "gvec_per_update")

    @property
    def rejected_updates(self):
        return 0 if self.tree is None else int(self._header()[PER_HDR_REJECTED])

    def _draw(self, batch_size, beta, u):
        """(indices, weights) of one call of gvec_per_sample; the caller holds `_guard`."""
        t = self._t
        idx = t.empty(batch_size, dtype=t.int64, device=self.device)
        w = t.empty(batch_size, dtype=t.float32, device=self.device)
        if u is not None:
            u = t.as_tensor(u, device=self.device).to(t.float64).reshape(-1).contiguous()
            if u.numel() != batch_size:
                raise ValueError(f"u has {u.numel()} entries for {batch_size} draws")
        check(self._L.gvec_per_sample(self.device.index, self._stream(), self.tree.data_ptr(), self.capacity, self.counters.data_ptr(),
                                      batch_size, self.beta if beta is None else float(beta), None if u is None else u.data_ptr(),
                                      self._seed, idx.data_ptr(), w.data_ptr()), "gvec_per_sample")
        return idx, w

    def sample_prioritized(self, batch_size, beta=None, u=None):
        """(states, actions, rewards, next_states, dones, indices, weights) as CUDA tensors: `batch_size` stratified draws
        with replacement, draw j aimed at (j + u[j]) / batch_size of the total priority; `u` (float64 in [0, 1), for
        reproducible tests) defaults to the kernel's counter RNG under `manual_seed`.  The draw and its gathers are enqueued
        under the collector's lock, like `sample_arrays`.  ValueError when the buffer is empty or holds fewer than
        batch_size transitions (the uniform buffer's contract)."""
        batch_size = self._checked(batch_size)
        with self._guard:
            idx, w = self._draw(batch_size, beta, u)
            return self.state[idx], self.action[idx], self.reward[idx], self.next_state[idx], self.done[idx], idx, w

    def sample_nstep_prioritized(self, batch_size, beta=None, u=None):
        """`sample_prioritized`'s draw with the n-step gather: (states, actions, returns, next_states, dones, discounts, steps,
        indices, weights).  `indices` are the chains' first slots - the ones `update_priorities` takes."""
        batch_size = self._checked(batch_size)
        with self._guard:
            idx, w = self._draw(batch_size, beta, u)
            return self._seven(self._gather_nstep(idx)) + (idx, w)

    def _checked(self, batch_size):
        batch_size = int(batch_size)
        held = len(self)
        if batch_size < 1 or batch_size > held or self.tree is None:
            raise ValueError("Sample larger than population or is negative" if held else "the replay buffer is empty")
        return batch_size

    def _sample_indices(self, batch_size):
        return self._draw(self._checked(batch_size), None, None)[0]

    def sample_indices(self, batch_size):
        """Prioritized, with replacement (the uniform buffer's are distinct); ValueError like `sample_prioritized`."""
        batch_size = self._checked(batch_size)
        with self._guard:
            return self._draw(batch_size, None, None)[0]

    def sample_arrays(self, batch_size):
        return self.sample_prioritized(batch_size)[:5]
