"""ParallelVecEnvPool — the collection surface `train_dqn_parallel.py` consumes, over ONE vector env.  The buffers it fills
are replay.py's; their three names stay importable from here.

Reference: python/generals_gym/vector_env.py:28-192 (ParallelEnvPool: N GeneralsEnv instances, one worker thread each,
every worker running whole episodes and pushing (state, action, reward, next_state, done) into a shared buffer).  Same
constructor keywords, same properties (`total_env_steps`, `total_episodes`, `alive_workers`), same `start / stop /
pop_episode_results`, same per-worker behaviour - the sequence of transitions worker w pushes and the (episode_reward,
episode_length, worker_id) results it reports are those of the reference's worker w given the same env behaviour and the
same `action_fn` (tests/test_env_pool.py replays fixtures recorded from the reference's own classes).

What differs, by construction of a vector env:
  * `env_factory(num_envs)` is called ONCE and returns the vector env (GeneralsVecEnv, numpy mode) - the reference calls
    `env_factory(worker_id)` once per worker;
  * one collector thread steps all "workers" (= env indices) in lock-step instead of N threads doing gRPC round trips;
  * an episode that ends (terminated / truncated, or cut at `max_steps_per_episode` - the pool then asks the env to
    re-deal that board with `force_reset`) starts its successor on the env's next step, which returns the new episode's
    first observation with info["reset"] set; that step is the worker's `env.reset()` and is not a transition;
  * with a `DeviceReplayBuffer` (and `GeneralsVecEnv(device_outputs=True)`, `batched_actions=True`) the whole loop is
    resident on the GPU: `action_fn(states, valid_masks, None, torch_generator) -> CUDA int64 actions[num_envs]`, transitions
    appended to the ring in HBM and episode results logged by `gvec_pool_collect` - the host only enqueues launches;
  * `batched_actions=True`: `action_fn(states[k], valid_masks[k], worker_ids[k], rngs) -> actions[k]` for the k workers
    that play this step (rngs: the list of all workers' RNGs, indexed by worker id) - one policy forward for all envs;
    the default keeps the reference's per-env signature `(state, valid_mask, worker_id, rng) -> int`
    with one private `random.Random(seed * 1000 + worker_id)` per worker (vector_env.py:138).

The pool owns the env, the thread and the retry loop; what a vector step does and what it keeps between steps is one of
two collectors', `_HostCollector` or `_DeviceCollector`, chosen once by the kind of buffer.  Both have the same four entries:
`restart(pool)` after the pool's `env.reset()`, `step(pool)`, `episodes`, `pop_results()`.
"""
import logging
import random
import threading
import time

import numpy as np

from ._lib import CollectArgs
from .replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer, ReplayBuffer  # noqa: F401 - re-exported

logger = logging.getLogger(__name__)


class _HostCollector:
    """The host form: numpy observations, `action_fn` on the host, `push` / `push_batch` into any reference-shaped buffer."""

    def __init__(self, num_envs, seed):
        self.num_envs = num_envs
        # private RNG per worker (vector_env.py:136-138): shared module-level RNGs would correlate exploration between workers
        self.rngs = [random.Random(seed * 1000 + w) for w in range(num_envs)]
        self.episode_reward = np.zeros(num_envs, np.float64)
        self.episode_length = np.zeros(num_envs, np.int64)
        self.starting = np.zeros(num_envs, bool)    # the worker's next vector step is its env.reset()
        self._tally = threading.Lock()              # guards the two fields below
        self._episodes = 0
        self._finished = []                         # (episode_reward, episode_length, worker_id) since the last pop

    def restart(self, pool):
        if pool._mask is None:
            pool._mask = np.ones((self.num_envs, pool._env.single_action_n), bool)
        self.episode_reward[:] = 0.0
        self.episode_length[:] = 0
        self.starting[:] = False

    def _actions(self, pool):
        """The policy is asked only for the workers that will play: a worker whose next step is its `env.reset()` chooses
        nothing (and draws nothing from its RNG), as in the reference's loop."""
        acts = np.zeros(self.num_envs, np.int64)
        idx = np.flatnonzero(~self.starting)
        if len(idx) == 0:
            return acts
        if pool.batched_actions:
            acts[idx] = np.asarray(pool.action_fn(pool._state[idx], pool._mask[idx], idx, self.rngs), np.int64).reshape(len(idx))
        else:
            for w in idx:
                acts[w] = pool.action_fn(pool._state[w], pool._mask[w], int(w), self.rngs[w])
        return acts

    def step(self, pool):
        """One vector step = one iteration of every worker's `_run_episode` loop (vector_env.py:172-192)."""
        state, env, buffer = pool._state, pool._env, pool.replay_buffer
        actions = self._actions(pool)
        next_state, reward, terminated, truncated, info = env.step(actions)
        reward = np.asarray(reward, np.float64)
        done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
        fresh = np.asarray(info.get("reset", np.zeros(self.num_envs, bool)), bool)   # this step was the worker's env.reset()
        live = ~fresh
        idx = np.flatnonzero(live)
        if len(idx):
            if hasattr(buffer, "push_batch"):
                if len(idx) == self.num_envs and getattr(buffer, "copies_what_it_is_given", False):
                    # the usual step: no worker is re-dealing, nothing to pick out - and this package's ring copies what it is
                    # given, so the env's own (soon reused) arrays can be handed over as they are
                    buffer.push_batch(state, actions, reward, next_state, done)
                else:
                    buffer.push_batch(np.array(state[idx]), actions[idx], reward[idx], np.array(next_state[idx]), done[idx])
            else:
                for w in idx:
                    buffer.push(np.array(state[w]), int(actions[w]), float(reward[w]), np.array(next_state[w]), bool(done[w]))
        self.episode_reward[live] += reward[live]
        self.episode_length[live] += 1
        over = live & (done | (self.episode_length >= pool.max_steps_per_episode))
        if over.any():
            ended = [(float(self.episode_reward[w]), int(self.episode_length[w]), int(w)) for w in np.flatnonzero(over)]
            with self._tally:
                self._episodes += len(ended)
                self._finished += ended
            cut = over & ~done
            if cut.any():
                env.force_reset(cut)            # the reference's next `env.reset()`: the env's own flags do not say so
            self.episode_reward[over] = 0.0
            self.episode_length[over] = 0
        self.starting = over
        pool._state = next_state
        m = info.get("valid_actions_mask")
        pool._mask = m if m is not None else np.ones((self.num_envs, env.single_action_n), bool)

    @property
    def episodes(self):
        with self._tally:
            return self._episodes

    def pop_results(self):
        with self._tally:
            out, self._finished = self._finished, []
        return out


class _DeviceCollector:
    """The resident form: env, policy and buffer all live on the GPU and the host only enqueues.  The episode count and the
    result log are the pool's for life (an env that is re-created after a failed step or a restart keeps what was counted and
    not yet read); what belongs to one env - accumulators, scratch, link state, the policy's generator - is made anew when
    `restart` meets another env."""

    def __init__(self, buffer, result_capacity):
        import torch
        self._t, self.buffer, self.env = torch, buffer, None
        self.result_capacity = n = int(result_capacity)
        z = self._zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device=buffer.device)
        self.result_reward, self.result_length, self.result_worker = z(n, torch.float64), z(n, torch.int32), z(n, torch.int32)
        self.counters = z(4, torch.int64)          # episodes, results held, results dropped, 0
        self._step_lock = threading.Lock()         # a vector step's launches vs. a reader of the result log

    def _bind(self, pool):
        env, buffer, torch, z = pool._env, self.buffer, self._t, self._zeros
        if not getattr(env, "device_outputs", False) or not pool.batched_actions:
            raise ValueError("a DeviceReplayBuffer needs a vector env with device_outputs=True and batched_actions=True")
        if buffer.device != env._dev:
            raise ValueError(f"replay buffer on {buffer.device}, env on {env._dev}")
        if buffer.capacity < env.num_envs:
            raise ValueError(f"a DeviceReplayBuffer must hold at least one vector step: capacity {buffer.capacity} < {env.num_envs} envs")
        buffer.allocate(env.single_observation_shape)
        n = env.num_envs
        self.episode_reward, self.episode_length = z(n, torch.float64), z(n, torch.int64)
        self.scratch = z((int(env.engine.L.gvec_pool_collect_scratch_bytes(n)) + 7) // 8, torch.int64)
        a = self.args = CollectArgs()
        a.num_envs, a.obs_floats, a.max_steps_per_episode = n, int(np.prod(env.single_observation_shape)), int(pool.max_steps_per_episode)
        a.capacity, a.result_capacity = buffer.capacity, self.result_capacity
        for name, tensor in buffer.ring_pointers() + (("episode_reward", self.episode_reward), ("episode_length", self.episode_length),
                                                      ("result_reward", self.result_reward), ("result_length", self.result_length),
                                                      ("result_worker", self.result_worker), ("pool_counters", self.counters),
                                                      ("scratch", self.scratch)):
            setattr(a, name, tensor.data_ptr())
        # n-step buffers: {sequence number, slot} of every worker's latest row while its episode is open; the ring's to use
        self.nstep_last = torch.full((n, 2), -1, dtype=torch.int64, device=env._dev) if buffer.n_step > 1 else None
        self.generator = torch.Generator(device=env._dev)      # the policy's, the fourth argument of `action_fn`
        self.generator.manual_seed(pool.seed)
        self.env = env

    def restart(self, pool):
        if self.env is not pool._env:
            self._bind(pool)
        self.episode_reward.zero_()
        self.episode_length.zero_()
        if self.nstep_last is not None:
            self.nstep_last.fill_(-1)             # a reopened env starts new episodes: nothing links across the gap

    def collect(self, state, actions, next_state, reward, terminated, truncated, was_reset, needs_reset):
        """The outputs of one env.step into the ring: the per-step pointers, then the ring's own append."""
        a = self.args
        a.state, a.next_state, a.action, a.reward = state.data_ptr(), next_state.data_ptr(), actions.data_ptr(), reward.data_ptr()
        a.terminated, a.truncated, a.was_reset, a.needs_reset = terminated.data_ptr(), truncated.data_ptr(), was_reset.data_ptr(), needs_reset.data_ptr()
        self.buffer.append_step(a, self._t.cuda.current_stream(self.env._dev).cuda_stream, self.nstep_last)

    def step(self, pool):
        """The same iteration with nothing on the host: the policy maps CUDA tensors to a CUDA int64 tensor of actions (it is
        asked for every worker; what it answers for a worker whose step is its `env.reset()` is ignored by the env), the gym
        kernel plays the step, gvec_pool_collect appends the transitions to the ring, keeps the episode accumulators, logs
        finished episodes and raises the env's needs_reset for episodes cut at `max_steps_per_episode`.  No synchronisation:
        the host only enqueues."""
        env = pool._env
        with self._step_lock:
            state = pool._state
            actions = pool.action_fn(state, pool._mask, None, self.generator)
            next_state, reward, terminated, truncated, info = env.step(actions)
            self.collect(state, env.last_actions, next_state, reward, terminated, truncated, info["reset"], env.needs_reset_buffer())
            pool._state, pool._mask = next_state, info["valid_actions_mask"]

    @property
    def episodes(self):
        return int(self.counters[0])

    def pop_results(self):
        with self._step_lock:                     # between two vector steps: the log is read and emptied in stream order
            held = int(self.counters[1])
            if held == 0:
                return []
            r, l, w = self.result_reward[:held].tolist(), self.result_length[:held].tolist(), self.result_worker[:held].tolist()
            self.counters[1] = 0
            return list(zip(r, l, w))


class ParallelVecEnvPool:
    """vector_env.py:28-192 over a vector env; see the module docstring for what is kept and what differs."""

    def __init__(self, num_envs, env_factory, action_fn, replay_buffer, max_steps_per_episode=200, max_env_retries=3, seed=42,
                 batched_actions=False, retry_sleep_s=2.0, result_capacity=1 << 20):
        # the reference's public attributes (vector_env.py:45-51)
        (self.num_envs, self.env_factory, self.action_fn, self.replay_buffer, self.max_steps_per_episode, self.max_env_retries,
         self.seed) = num_envs, env_factory, action_fn, replay_buffer, max_steps_per_episode, max_env_retries, seed
        self.batched_actions, self.retry_sleep_s = bool(batched_actions), retry_sleep_s
        self.result_capacity = int(result_capacity)
        # a DeviceReplayBuffer switches the pool to its resident form: env (device_outputs), policy and ring on the GPU
        self._dc = _DeviceCollector(replay_buffer, self.result_capacity) if isinstance(replay_buffer, DeviceReplayBuffer) else None
        self._steps = self._dc or _HostCollector(num_envs, seed)   # what a vector step does, and its bookkeeping
        self.on_device = self._dc is not None
        # one collector thread instead of one thread per env
        self._halt = threading.Event()
        self._collector = None
        self._tally = threading.Lock()          # guards _live
        self._live = 0
        self._env = None
        self._state = self._mask = None

    # ---- the reference's public surface (vector_env.py:62-112) ----------------------------------------------
    def start(self):
        """Starts the collector (a daemon thread) for all environments."""
        if self._collector is not None:
            raise RuntimeError("Pool already started")
        self._halt.clear()
        with self._tally:
            self._live = self.num_envs
        self._collector = threading.Thread(target=self._worker_loop, name="env-worker-vec", daemon=True)
        self._collector.start()
        logger.info("collector started for %d envs", self.num_envs)

    def stop(self, join_timeout=10.0):
        """Asks the collector to finish its current vector step and waits for it; a straggler is logged, not raised
        (the thread is a daemon)."""
        self._halt.set()
        t, self._collector = self._collector, None
        if t is not None:
            t.join(timeout=join_timeout)
            if t.is_alive():
                logger.warning("collector %s still running after %.1fs", t.name, join_timeout)

    @property
    def total_env_steps(self):
        return self.replay_buffer.total_pushed      # one transition pushed == one environment step

    @property
    def total_episodes(self):
        return self._steps.episodes

    @property
    def alive_workers(self):
        with self._tally:
            return self._live

    def pop_episode_results(self):
        """Finished-episode results since the last call, oldest first."""
        return self._steps.pop_results()

    # ---- collection ---------------------------------------------------------------------------------------------
    def _create_env(self, old_env=None):
        """Opens the vector env, closing a broken predecessor first; up to max_env_retries tries, retry_sleep_s apart
        (the reference's pattern, vector_env.py:114-134)."""
        if old_env is not None:
            try:
                old_env.close()
            except Exception:  # noqa: BLE001 - it is being replaced anyway
                pass
        tries = 0
        while True:
            tries += 1
            try:
                env = self._open_env()
            except Exception as e:  # noqa: BLE001
                logger.warning("opening the vector environment failed (%d of %d): %s", tries, self.max_env_retries, e)
                if tries >= self.max_env_retries:
                    raise RuntimeError("failed to create the vector environment") from e
                time.sleep(self.retry_sleep_s)
            else:
                logger.info("vector environment open")
                return env

    def _open_env(self):
        return self.env_factory(self.num_envs)

    def _begin(self):
        """Every worker's first `env.reset()` (vector_env.py:166-167)."""
        self._state, info = self._env.reset()
        self._mask = info.get("valid_actions_mask")
        self._steps.restart(self)

    def collect(self, steps):
        """Synchronous form for trainers and tests that own the loop: `steps` vector steps in the caller's thread."""
        if self._env is None:
            self._env = self._create_env()
            self._begin()
        for _ in range(steps):
            self._steps.step(self)

    def _worker_loop(self):
        """The collector thread: vector steps until stop(); a step that raises costs the running episodes (like a failed
        worker episode in the reference) and the env is reopened; when reopening fails for good the collector ends and
        alive_workers drops to 0."""
        try:
            if self._env is None:
                self._env = self._create_env()
                self._begin()
            while not self._halt.is_set():
                try:
                    self._steps.step(self)
                except Exception as e:  # noqa: BLE001
                    if self._halt.is_set():
                        break
                    logger.warning("vector step failed: %s", e)
                    self._env = self._create_env(old_env=self._env)
                    self._begin()
        except Exception as e:  # noqa: BLE001
            logger.error("collector ends: %s", e)
        finally:
            env, self._env = self._env, None
            if env is not None:
                try:
                    env.close()
                except Exception:  # noqa: BLE001
                    pass
            with self._tally:
                self._live = 0
