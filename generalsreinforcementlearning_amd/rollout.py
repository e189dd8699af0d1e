"""SelfPlayRolloutBuffer — on-policy (PPO) collection from GeneralsSelfPlayVecEnv without leaving the device.

A rollout is `horizon` = T steps of N = num_envs * num_learners streams ([B][L], learner-minor, as the env emits them).  The
buffer owns every store in HBM: observations and masks of T + 1 slots (the env's step launch writes slot t + 1 directly: no
second copy of the 8 to 14 KB rows), action / log-prob / value / reward / flags per row, and after `finish` advantages and
returns.  Four HIP entry points do the work (include/generals_vec.h): gvec_traj_record (one launch
per step), gvec_traj_gae, gvec_traj_compact, gvec_traj_gather.  A fifth, gvec_traj_vtrace, replaces
gvec_traj_gae where the network that learns is no longer the one that acted: `finish_vtrace`, fed by `evaluate_rollout`.

The episode protocol, which the flags of a row encode (TRAJ_VALID / TRAJ_TERMINAL / TRAJ_CUT):
  - a step that re-dealt its env (info["reset"]) is no transition: the action was ignored - its rows are invalid;
  - a learner that was eliminated before the step has no transition - invalid; the step that eliminates it is terminal for it;
  - a truncated episode bootstraps from the value of its final observation: that observation is slot t + 1, the row after
    it is the env's re-deal row, so value[t + 1] is exactly the bootstrap and no special case exists.
Precondition: every board holds max_players players (GeneralsSelfPlayVecEnv always deals such boards).

    buf = SelfPlayRolloutBuffer(env, horizon=128)
    buf.begin(*env.reset())
    while training:
        while not buf.full:
            actions, logp, value = policy(buf.obs, buf.valid_actions_mask)
            buf.step(actions, logp, value)
        buf.finish(policy.value(buf.obs))
        for batch in buf.minibatches(4096, epochs=4):
            ...                      # batch["weight"] is 0 for the invalid rows
        buf.next_rollout()

Off-policy (a lagging actor, or every epoch after the first gradient step): V-trace targets instead of GAE's, from the
learner's own log-probs and values of the stored rows, re-evaluated in place:

        for epoch in range(4):
            logp, value = buf.evaluate_rollout(lambda obs, memory: net(obs), head)      # net: obs -> (logits, value)
            buf.finish_vtrace(net(buf.obs.flatten(0, 1))[1], logp, value=value)
            for batch in buf.minibatches(4096):
                ...                  # batch["rho"] is the clipped importance weight of the row

Nothing here synchronises with the host, except minibatches(compact=True): one 8-byte read per rollout.

memory=ObservationMemory((num_envs, num_learners), H, W) carries the fog-of-war memory planes (memory.py, DESIGN.md section
4.14) along: every step's update writes straight into slot t + 1 of a store beside the observations', `buf.memory` is the
current slot's view and every batch has a "memory" entry.  Without it nothing is allocated or launched.

policy_target=True keeps what a search says about every step beside what the actor did: a float32
target over the 5 * H * W actions of a row and the search's value, given to `step`, returned by `gather` as
batch["policy_target"] / batch["search_value"] and consumed by MaskedCategoricalHead.distill / distill_loss.  target_store is
float32 [T, N, 5 * H * W]: one more mask store times four (4 bytes per action where the mask has one; 18.4 MB per step at
4,096 streams on 15x15).  `buf.policy_target_slot` is slot t's view, for a search that writes there directly.  Without it
nothing is allocated, launched or added to any batch.
"""
import ctypes as C

from ._lib import TRAJ_VALID, TrajCompactArgs, TrajGaeArgs, TrajGatherArgs, TrajRecordArgs, TrajVtraceArgs, check, load


class SelfPlayRolloutBuffer:
    def __init__(self, env, horizon, gamma=0.99, gae_lambda=0.95, memory=None, policy_target=False):
        import torch
        if not getattr(env, "device_outputs", False):
            raise ValueError("SelfPlayRolloutBuffer needs an env built with device_outputs=True")
        if horizon < 1:
            raise ValueError(f"horizon must be >= 1: {horizon}")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= gae_lambda <= 1.0):
            raise ValueError(f"gamma and gae_lambda must lie in [0, 1]: {gamma}, {gae_lambda}")
        want = ((env.num_envs, env.num_learners), env.board_height, env.board_width)
        if memory is not None and (getattr(memory, "rows_shape", None), getattr(memory, "height", None), getattr(memory, "width", None)) != want:
            raise ValueError(f"memory must be an ObservationMemory of rows_shape {want[0]} on a {want[2]}x{want[1]} board")
        if not isinstance(policy_target, bool):
            raise ValueError(f"policy_target must be True or False: {policy_target!r}")
        self._t = t = torch
        self.env = env
        self.horizon = T = int(horizon)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.num_envs, self.num_learners = B, L = env.num_envs, env.num_learners
        self.num_streams = N = B * L
        self._dev = dev = env._dev
        self._L = load()
        H, W, nb = env.board_height, env.board_width, env.board_size
        self.obs_floats, self.mask_bytes, self.mem_floats = 9 * nb, 5 * nb, 4 * nb
        z = lambda shape, dt: t.zeros(shape, dtype=dt, device=dev)
        self.obs_store = z((T + 1, B, L, 9, H, W), t.float32)
        self.mask_store = z((T + 1, B, L, 5 * nb), t.uint8)
        self.action, self.logp, self.value = z((T, N), t.int64), z((T, N), t.float32), z((T + 1, N), t.float32)
        self.reward, self.flags = z((T, N), t.float64), z((T, N), t.uint8)
        self._adv, self._ret = z((T, N), t.float32), z((T, N), t.float32)
        self.stats = z(4, t.float64)
        self.alive_state = t.ones(N, dtype=t.uint8, device=dev)
        self._scratch = z(int(self._L.gvec_traj_scratch_bytes(T, N)), t.uint8)
        self._idx, self._count, self.rejected = None, z(1, t.int64), z(1, t.int64)
        self._valid_count = None
        self._out = {}
        self._step = 0
        self._finished = False
        self._rec = TrajRecordArgs(T=T, t=0, num_envs=B, num_learners=L, alive_state=self.alive_state.data_ptr(),
                                   action=self.action.data_ptr(), logp=self.logp.data_ptr(), value=self.value.data_ptr(),
                                   reward=self.reward.data_ptr(), flags=self.flags.data_ptr())
        self._rec_ref = C.byref(self._rec)
        self._memory = memory
        self.mem_store = None if memory is None else z((T + 1, N, 4, nb), t.float32)
        self._rho = self._vt_value = None                               # V-trace's stores: allocated by the first finish_vtrace
        self._vtrace = False
        self._has_target = policy_target
        self.target_store = z((T, N, 5 * nb), t.float32) if policy_target else None
        self.search_value_store = z((T, N), t.float32) if policy_target else None

    # ---- collection ---------------------------------------------------------------------------------------------------
    def _stream(self):
        return self._t.cuda.current_stream(self._dev).cuda_stream

    @property
    def full(self):
        return self._step >= self.horizon

    @property
    def obs(self):
        """The current observation [B, L, 9, H, W]: a view of slot t."""
        return self.obs_store[self._step]

    @property
    def memory(self):
        """The memory planes of the current observation [B, L, 4, H, W]: a view of slot t (None without memory=)."""
        if self.mem_store is None:
            return None
        return self.mem_store[self._step].view(self._memory.shape)

    @property
    def valid_actions_mask(self):
        return self.mask_store[self._step].view(self._t.bool)

    @property
    def policy_target_slot(self):
        """Where the current step's policy target goes [B, L, 5 * H * W]: a view of slot t (None without policy_target=True).
        A target written here and then handed to `step` is not copied again."""
        if self.target_store is None:
            return None
        if self.full:
            raise RuntimeError(f"the rollout is full ({self.horizon} steps): there is no slot {self._step}")
        return self.target_store[self._step].view(self.num_envs, self.num_learners, -1)

    def _take_target(self, policy_target, search_value):
        """step's two optional arguments, checked: every ValueError comes before anything is launched or stored."""
        t = self._t
        if not self._has_target:
            if policy_target is not None or search_value is not None:
                raise ValueError("step() got a policy_target / search_value, but the buffer was built with policy_target=False")
            return None
        if policy_target is None:
            raise ValueError("the buffer was built with policy_target=True: step() needs the step's policy_target")
        A = self.mask_bytes
        if not isinstance(policy_target, t.Tensor) or policy_target.dtype != t.float32 or policy_target.dim() < 1 \
                or policy_target.shape[-1] != A or policy_target.numel() != self.num_streams * A:
            raise ValueError(f"policy_target must be a float32 tensor [{self.num_envs}, {self.num_learners}, {A}]")
        if search_value is not None and (not isinstance(search_value, t.Tensor) or search_value.numel() != self.num_streams):
            raise ValueError(f"search_value must be a tensor of {self.num_envs} x {self.num_learners} elements")
        return policy_target, search_value

    def _store_target(self, k, policy_target, search_value):
        row = self.target_store[k]
        same = policy_target.device == row.device and policy_target.data_ptr() == row.data_ptr() and policy_target.is_contiguous()
        if not same:                                                    # the slot's own view was written in place: nothing to copy
            row.copy_(policy_target.reshape(row.shape))
        if search_value is None:
            self.search_value_store[k].zero_()
        else:
            self.search_value_store[k].copy_(search_value.reshape(-1))

    def begin(self, obs, info):
        """After env.reset(): slot 0 takes the observation and the mask, every learner is alive."""
        self.obs_store[0].copy_(obs)
        self.mask_store[0].copy_(info["valid_actions_mask"].view(self._t.uint8))
        self.alive_state.fill_(1)
        if self._memory is not None:
            self._memory.reset_all()
            self._memory.update(self.obs_store[0], out=self.mem_store[0])
        self._restart()

    def _restart(self):
        self._step, self._finished, self._valid_count, self._vtrace = 0, False, None, False

    def _as(self, x, dtype):
        t = self._t
        if not (isinstance(x, t.Tensor) and x.is_cuda and x.dtype == dtype and x.is_contiguous() and x.numel() == self.num_streams):
            x = t.as_tensor(x, dtype=dtype).to(self._dev).reshape(self.num_streams).contiguous()
        return x

    def step(self, actions, logp, value, policy_target=None, search_value=None):
        """env.step(actions) with the observation and mask written into slot t + 1, then row t of the small stores in one
        launch.  actions int64, logp / value float32, [B, L] each (CUDA, contiguous: anything else is converted first).
        On a buffer built with policy_target=True: policy_target float32 [B, L, 5 * H * W] (required) and search_value
        [B, L] (optional: zeros) go into row t of target_store / search_value_store; `policy_target_slot` itself is not copied.
        Returns the env's tuple."""
        target = self._take_target(policy_target, search_value)
        k = self._step
        if k >= self.horizon:
            raise RuntimeError(f"the rollout is full ({self.horizon} steps): finish() and next_rollout() come first")
        t = self._t
        if target is not None:
            self._store_target(k, *target)
        actions, logp, value = self._as(actions, t.int64), self._as(logp, t.float32), self._as(value, t.float32)
        out = self.env.step(actions, obs_out=self.obs_store[k + 1], mask_out=self.mask_store[k + 1])
        _, reward, terminated, truncated, info = out
        r = self._rec
        r.t = k
        r.step_action, r.step_logp, r.step_value, r.step_reward = actions.data_ptr(), logp.data_ptr(), value.data_ptr(), reward.data_ptr()
        r.reset, r.terminated, r.truncated, r.alive = (info["reset"].data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                                                       info["alive"].data_ptr())
        check(self._L.gvec_traj_record(self._dev.index, self._stream(), self._rec_ref), "gvec_traj_record")
        if self._memory is not None:                                    # a re-dealt env's rows restart from blank
            self._memory.update(self.obs_store[k + 1], info["reset"], out=self.mem_store[k + 1])
        self._step = k + 1
        return out

    def finish(self, last_value):
        """last_value [B, L]: the value of the current observation (slot T), the bootstrap of every stream still running.
        Runs gvec_traj_gae; afterwards advantages / returns / valid / stats are set."""
        if not self.full:
            raise RuntimeError(f"finish() after {self._step} of {self.horizon} steps")
        T, N = self.horizon, self.num_streams
        self.value[T].copy_(self._as(last_value, self._t.float32).view(-1))
        a = TrajGaeArgs(T=T, N=N, gamma=self.gamma, lam=self.gae_lambda, reward=self.reward.data_ptr(), value=self.value.data_ptr(),
                        flags=self.flags.data_ptr(), adv=self._adv.data_ptr(), ret=self._ret.data_ptr(), stats=self.stats.data_ptr(),
                        scratch=self._scratch.data_ptr())
        check(self._L.gvec_traj_gae(self._dev.index, self._stream(), C.byref(a)), "gvec_traj_gae")
        self._finished, self._vtrace = True, False

    def finish_vtrace(self, last_value, target_logp, value=None, rho_bar=1.0, c_bar=1.0):
        """V-trace targets (gvec_traj_vtrace) in place of GAE's, for a rollout whose actor is not the network being trained.
        target_logp float32 [T, B, L] (or [T, N]): the learner's log-prob of every stored action, as `evaluate_rollout`
        returns it; the stored `logp` is the behaviour's.  value [T, B, L], optional: the learner's fresh values of slots
        0 .. T-1, which with last_value go into a store of the buffer's own - the recorded `self.value` stays as it is and
        batch["value"] still returns it.  Without it the recorded values are used, as finish() uses them.
        Afterwards advantages is pg, returns is vs, stats is {valid rows, sum pg, sum pg^2, sum rho}, `rho` [T, B, L] holds
        min(rho_bar, pi / mu) (0 on invalid rows) and every batch has a "rho" entry.  It may be called again on the same
        rollout (re-targeting between epochs), and finish() after it restores the GAE outputs.  No host sync."""
        if not self.full:
            raise RuntimeError(f"finish_vtrace() after {self._step} of {self.horizon} steps")
        t, T, N = self._t, self.horizon, self.num_streams
        if not (float(rho_bar) > 0.0 and float(c_bar) > 0.0):
            raise ValueError(f"rho_bar and c_bar must be > 0: {rho_bar}, {c_bar}")

        def rows(x, name):
            if not isinstance(x, t.Tensor) or x.numel() != T * N:
                raise ValueError(f"{name} must be a tensor of {T} x {self.num_envs} x {self.num_learners} elements")
            if not (x.is_cuda and x.dtype == t.float32 and x.is_contiguous()):
                x = x.to(device=self._dev, dtype=t.float32).contiguous()
            return x.view(T, N)

        target_logp = rows(target_logp, "target_logp")
        last_value = self._as(last_value, t.float32).view(-1)
        if value is None:
            values = self.value
        else:
            if self._vt_value is None:
                self._vt_value = t.zeros((T + 1, N), dtype=t.float32, device=self._dev)
            values = self._vt_value
            values[:T].copy_(rows(value, "value"))
        values[T].copy_(last_value)
        if self._rho is None:
            self._rho = t.zeros((T, N), dtype=t.float32, device=self._dev)
        a = TrajVtraceArgs(T=T, N=N, gamma=self.gamma, lam=self.gae_lambda, rho_bar=float(rho_bar), c_bar=float(c_bar),
                           reward=self.reward.data_ptr(), value=values.data_ptr(), flags=self.flags.data_ptr(),
                           logp_behaviour=self.logp.data_ptr(), logp_target=target_logp.data_ptr(), vs=self._ret.data_ptr(),
                           pg=self._adv.data_ptr(), rho_out=self._rho.data_ptr(), stats=self.stats.data_ptr(),
                           scratch=self._scratch.data_ptr())
        check(self._L.gvec_traj_vtrace(self._dev.index, self._stream(), C.byref(a)), "gvec_traj_vtrace")
        self._finished = self._vtrace = True

    def evaluate_rollout(self, fn, head, chunk_rows=None):
        """The learner's view of the stored rollout, without gathering it: fn(obs [M, 9, H, W], memory [M, 4, H, W] or None)
        -> (logits [M, A], value [M]) is called on contiguous chunks of rows 0 .. T * N of the stores (views: no gather, no
        copy; chunk_rows=None takes them all at once), under torch.no_grad(), and head.evaluate scores the stored actions
        under the stored masks.  Returns (logp [T, B, L], value [T, B, L]), what finish_vtrace takes."""
        t, env = self._t, self.env
        total = self.horizon * self.num_streams
        chunk = total if chunk_rows is None else int(chunk_rows)
        if chunk < 1:
            raise ValueError(f"chunk_rows must be >= 1: {chunk_rows}")
        obs = self.obs_store.view(-1, 9, env.board_height, env.board_width)
        mask = self.mask_store.view(-1, self.mask_bytes).view(t.bool)
        mem = None if self.mem_store is None else self.mem_store.view(-1, 4, env.board_height, env.board_width)
        action = self.action.view(-1)
        logp, value = t.empty(total, dtype=t.float32, device=self._dev), t.empty(total, dtype=t.float32, device=self._dev)
        with t.no_grad():
            for lo in range(0, total, chunk):
                hi = min(lo + chunk, total)
                logits, v = fn(obs[lo:hi], None if mem is None else mem[lo:hi])
                lp, _ = head.evaluate(logits, mask[lo:hi], action[lo:hi])
                logp[lo:hi].copy_(lp.view(-1))
                value[lo:hi].copy_(v.reshape(-1))
        shape = (self.horizon, self.num_envs, self.num_learners)
        return logp.view(shape), value.view(shape)

    def _done(self):
        if not self._finished:
            raise RuntimeError("advantages exist after finish()")
        return (self.horizon, self.num_envs, self.num_learners)

    @property
    def advantages(self):
        return self._adv.view(self._done())

    @property
    def returns(self):
        return self._ret.view(self._done())

    @property
    def rho(self):
        """[T, B, L]: the clipped importance weights of the last finish_vtrace (0 on invalid rows)."""
        if not self._vtrace:
            raise RuntimeError("rho exists after finish_vtrace()")
        return self._rho.view(self._done())

    @property
    def valid(self):
        return (self.flags & TRAJ_VALID).bool().view(self._done())

    # ---- minibatches ----------------------------------------------------------------------------------------------------
    def _outputs(self, m):
        o = self._out.get(m)
        if o is None:
            t, env = self._t, self.env
            e = lambda shape, dt: t.empty(shape, dtype=dt, device=self._dev)
            o = self._out[m] = {"obs": e((m, 9, env.board_height, env.board_width), t.float32), "mask": e((m, self.mask_bytes), t.uint8),
                                "action": e(m, t.int64), "logp": e(m, t.float32), "value": e(m, t.float32), "ret": e(m, t.float32),
                                "adv": e(m, t.float32), "weight": e(m, t.float32)}
            if self.mem_store is not None:
                o["memory"] = e((m, 4, env.board_height, env.board_width), t.float32)
            if self._has_target:
                o["policy_target"], o["search_value"] = e((m, self.mask_bytes), t.float32), e(m, t.float32)
        return o

    def gather(self, pos, normalize=True):
        """The rows at positions pos (int64 CUDA tensor [M], p = t * N + b * L + l) as one batch: a dict of obs [M, 9, H, W],
        valid_actions_mask bool [M, 5 * H * W], action, logp, value, returns, advantages (normalised over the rollout's valid
        rows when `normalize`) and weight (1 for a valid row, 0 otherwise) [M].  The tensors are reused by the next gather of
        the same M.  With memory=: also memory [M, 4, H, W], the planes stored at the same positions (a position outside the
        rollout, which `rejected` counts and whose weight is 0, gets those of the nearest row).  After finish_vtrace: also rho [M],
        fetched the same way.  With policy_target=True: also policy_target float32 [M, 5 * H * W] and search_value [M], the
        rows of target_store / search_value_store at the same (clamped) positions."""
        self._done()
        m = int(pos.numel())
        o = self._outputs(m)
        a = TrajGatherArgs(T=self.horizon, N=self.num_streams, M=m, obs_floats=self.obs_floats, mask_bytes=self.mask_bytes,
                           pos=pos.data_ptr(), obs=self.obs_store.data_ptr(), mask=self.mask_store.data_ptr(), action=self.action.data_ptr(),
                           logp=self.logp.data_ptr(), value=self.value.data_ptr(), ret=self._ret.data_ptr(), adv=self._adv.data_ptr(),
                           flags=self.flags.data_ptr(), stats=self.stats.data_ptr() if normalize else None, out_obs=o["obs"].data_ptr(),
                           out_mask=o["mask"].data_ptr(), out_action=o["action"].data_ptr(), out_logp=o["logp"].data_ptr(),
                           out_value=o["value"].data_ptr(), out_ret=o["ret"].data_ptr(), out_adv=o["adv"].data_ptr(),
                           out_weight=o["weight"].data_ptr(), rejected=self.rejected.data_ptr())
        check(self._L.gvec_traj_gather(self._dev.index, self._stream(), C.byref(a)), "gvec_traj_gather")
        batch = {"obs": o["obs"], "valid_actions_mask": o["mask"].view(self._t.bool), "action": o["action"], "logp": o["logp"],
                 "value": o["value"], "returns": o["ret"], "advantages": o["adv"], "weight": o["weight"], "index": pos}
        if self.mem_store is not None:
            rows = self.mem_store.view(-1, self.mem_floats)[:self.horizon * self.num_streams]
            self._t.index_select(rows, 0, pos.clamp(0, rows.shape[0] - 1), out=o["memory"].view(m, self.mem_floats))
            batch["memory"] = o["memory"]
        if self._has_target:
            rows = self.target_store.view(-1, self.mask_bytes)
            at = pos.clamp(0, rows.shape[0] - 1)
            self._t.index_select(rows, 0, at, out=o["policy_target"])
            self._t.index_select(self.search_value_store.view(-1), 0, at, out=o["search_value"])
            batch["policy_target"], batch["search_value"] = o["policy_target"], o["search_value"]
        if self._vtrace:
            if "rho" not in o:
                o["rho"] = self._t.empty(m, dtype=self._t.float32, device=self._dev)
            self._t.index_select(self._rho.view(-1), 0, pos.clamp(0, self._rho.numel() - 1), out=o["rho"])
            batch["rho"] = o["rho"]
        return batch

    def valid_positions(self):
        """(idx, count): the ascending positions of the valid rows in idx[:count] (gvec_traj_compact), count a Python int -
        the one host read of a rollout, made once and remembered until the next rollout."""
        self._done()
        t = self._t
        if self._valid_count is None:
            T, N = self.horizon, self.num_streams
            if self._idx is None:
                self._idx = t.empty(T * N, dtype=t.int64, device=self._dev)
            a = TrajCompactArgs(T=T, N=N, flags=self.flags.data_ptr(), idx=self._idx.data_ptr(), count=self._count.data_ptr(),
                                scratch=self._scratch.data_ptr())
            check(self._L.gvec_traj_compact(self._dev.index, self._stream(), C.byref(a)), "gvec_traj_compact")
            self._valid_count = int(self._count.item())
        return self._idx, self._valid_count

    def minibatches(self, batch_size, epochs=1, normalize=True, compact=False, seed=None):
        """Yields `epochs` shuffled passes over the rollout in batches of batch_size rows (the last of a pass may be shorter).
        compact=False  permutes all T * N rows: no host sync at all; invalid rows come with weight 0 (multiply the loss by
                       it) and cost their share of the batch - a few percent at long episodes, more when max_turns is short.
        compact=True   permutes only the valid rows: every row of every batch counts, at the price of one 8-byte read of
                       their number per rollout (the host needs it to size the batches)."""
        t = self._t
        self._done()
        gen = None
        if seed is not None:
            gen = t.Generator(device=self._dev)
            gen.manual_seed(int(seed))
        if compact:
            idx, total = self.valid_positions()
        else:
            idx, total = None, self.horizon * self.num_streams
        for _ in range(epochs):
            perm = t.randperm(total, device=self._dev, generator=gen)
            if idx is not None:
                perm = idx[perm]
            for lo in range(0, total, batch_size):
                yield self.gather(perm[lo:lo + batch_size], normalize)

    def next_rollout(self):
        """Slot T becomes slot 0 (one slot's copy); alive_state carries over; the stores are reused."""
        T = self.horizon
        self.obs_store[0].copy_(self.obs_store[T])
        self.mask_store[0].copy_(self.mask_store[T])
        if self._memory is not None:
            self._memory.move_to(self.mem_store[0])                     # its planes are slot T's: the last step wrote them there
        self._restart()
