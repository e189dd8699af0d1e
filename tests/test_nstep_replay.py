"""n-step returns on the device replay ring (gvec_nstep_link, gvec_nstep_gather, the buffers' n_step keyword)
against the numpy model of _nstep_reference.py.  Returns and discounts are compared bit for bit: the kernel's float64 walk
has no fused multiply-add, so numpy's float64 loop is its exact model."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import _nstep_reference as N
import _per_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEP = ["gvec_nstep_link", "gvec_nstep_gather"]
ENVS, STEPS, LIMIT = 130, 20, 7            # three 64-worker groups with a ragged tail


# ---- without a GPU ----------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_documented():
    from generalsreinforcementlearning_amd import _lib
    import generalsreinforcementlearning_amd as g
    hdr = open(os.path.join(ROOT, "include", "generals_vec.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = g.load()
    for name in NSTEP:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in doc, name
    assert "gvec_nstep_gather_args" in hdr
    assert g.DeviceReplayBuffer is not None and g.PrioritizedDeviceReplayBuffer is not None


def _gather_args(**kw):
    from generalsreinforcementlearning_amd._lib import NstepGatherArgs
    a = NstepGatherArgs()
    a.k, a.capacity, a.n_step, a.obs_floats, a.gamma = 4, 100, 3, 3, 0.99
    for name, _ in NstepGatherArgs._fields_[5:]:
        setattr(a, name, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _collect_args(**kw):
    from generalsreinforcementlearning_amd._lib import CollectArgs
    a = CollectArgs()
    a.num_envs, a.obs_floats, a.max_steps_per_episode, a.capacity, a.result_capacity = 8, 3, 5, 100, 0
    for name, typ in CollectArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_need_no_device():
    import generalsreinforcementlearning_amd as g
    L = g.load()
    p = C.c_void_p(4096)
    inv = lambda rc, word: rc == -1 and word in L.gvec_last_error()
    G = lambda **kw: L.gvec_nstep_gather(0, None, C.byref(_gather_args(**kw)))
    assert inv(L.gvec_nstep_gather(0, None, None), b"NULL")
    assert inv(G(capacity=0), b"capacity")
    assert inv(G(k=-1), b"k -1")
    assert inv(G(n_step=0), b"n_step")
    assert inv(G(obs_floats=0), b"obs_floats")
    for gamma in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert inv(G(gamma=gamma), b"gamma")
    assert inv(G(ring_succ=None), b"ring_succ")
    assert inv(G(ring_succ=None, n_step=2), b"ring_succ")
    for name in ("idx", "ring_state", "ring_next_state", "ring_action", "ring_reward", "ring_done", "ring_counters", "state", "next_state",
                 "action", "ret", "discount", "done", "steps", "last_idx"):
        assert inv(G(**{name: None}), b"NULL"), name
    assert inv(G(ring_succ=None, n_step=1, idx=None), b"NULL")       # gets past the ring_succ check: NULL is allowed there
    K = lambda a, before=p, succ=p, last=p: L.gvec_nstep_link(0, None, a, before, succ, last)
    assert inv(K(None), b"NULL")
    assert inv(K(C.byref(_collect_args()), before=None), b"NULL")
    assert inv(K(C.byref(_collect_args()), succ=None), b"NULL")
    assert inv(K(C.byref(_collect_args()), last=None), b"NULL")
    assert inv(K(C.byref(_collect_args(capacity=0))), b"capacity")
    assert inv(K(C.byref(_collect_args(num_envs=0))), b"num_envs")
    assert inv(K(C.byref(_collect_args(num_envs=101))), b"num_envs")
    for name in ("ring_counters", "scratch"):
        assert inv(K(C.byref(_collect_args(**{name: None}))), b"NULL"), name
    assert inv(K(C.byref(_collect_args(scratch=4096 + 8))), b"aligned")


def test_k_zero_is_a_no_op_without_a_device():
    import generalsreinforcementlearning_amd as g
    L = g.load()
    assert L.gvec_nstep_gather(0, None, C.byref(_gather_args(k=0))) == 0
    assert L.gvec_nstep_gather(0, None, C.byref(_gather_args(k=0, idx=None, state=None, ring_succ=None, n_step=1))) == 0


def test_python_keywords_are_checked_without_a_device():
    import inspect
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["n_step"].default == 1 and sig["gamma"].default == 0.99
        for m in ("gather_nstep", "sample_nstep"):
            assert callable(getattr(cls, m))
    assert list(inspect.signature(DeviceReplayBuffer.__init__).parameters)[1:5] == ["capacity", "device", "n_step", "gamma"]
    assert callable(PrioritizedDeviceReplayBuffer.sample_nstep_prioritized)
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):      # refused before torch touches a device
        for kw in ({"n_step": 0}, {"n_step": -3}, {"n_step": 2.5}, {"gamma": -0.1}, {"gamma": float("nan")}, {"gamma": float("inf")}):
            with pytest.raises(ValueError):
                cls(100, **kw)


@pytest.fixture(scope="module")
def models():
    """The model rings of the link test, by capacity (observations of three floats)."""
    return {cap: N.run(ENVS, cap, STEPS, LIMIT, 3) for cap in (1043, 131, 130)}


def test_model_inputs_exercise_every_path(models):
    sc, m = models[1043]
    assert m.total > 1043 == m.size                                    # wraps once
    assert m.full_chain_fraction(3) >= 0.40
    assert m.ended_by_done >= 50 and m.ended_by_cut >= 50
    for cap in (131, 130):
        assert models[cap][1].skipped_links >= 1000, cap


@pytest.mark.parametrize("case", [(ENVS, 1043, STEPS, LIMIT), (ENVS, 131, STEPS, LIMIT), (ENVS, 130, STEPS, LIMIT), (5, 23, 30, 4)])
def test_model_walks_agree(case):
    """The brute-force walk over the (worker, episode, t) tags and the walk over the links give the same batches."""
    n, cap, steps, limit = case
    sc, m = N.run(n, cap, steps, limit, 3)
    idx = np.arange(-1, m.size + 1)
    for n_step in (1, 2, 3, 5):
        a, b = m.gather(idx, n_step, 0.99, "links"), m.gather(idx, n_step, 0.99, "tags")
        for f in a:
            assert np.array_equal(a[f], b[f]), (case, n_step, f)
    one = m.gather(idx, 1, 0.5)
    assert np.array_equal(one["ret"][1:-1], m.reward[:m.size]) and (one["discount"][1:-1] == 0.5).all()


# ---- on the GPU ----------------------------------------------------------------------------------------------------
class _Ring:
    """A replay ring and a collector's device state, driven through the handle-free ABI with synthetic per-step tensors."""

    def __init__(self, num_envs, capacity, limit, obs_floats):
        import torch
        import generalsreinforcementlearning_amd as g
        from generalsreinforcementlearning_amd._lib import CollectArgs
        self.t, self.L, self.n, self.cap, self.F = torch, g.load(), num_envs, capacity, obs_floats
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.state, self.next_state = z((capacity, obs_floats), torch.float32), z((capacity, obs_floats), torch.float32)
        self.action, self.reward, self.done = z(capacity, torch.int64), z(capacity, torch.float64), z(capacity, torch.uint8)
        self.counters, self.before, self.pool_counters = z(4, torch.int64), z(4, torch.int64), z(4, torch.int64)
        self.succ = torch.full((capacity,), -1, dtype=torch.int64, device="cuda")
        self.last = torch.full((num_envs, 2), -1, dtype=torch.int64, device="cuda")
        self.ep_reward, self.ep_length = z(num_envs, torch.float64), z(num_envs, torch.int64)
        self.needs_reset = z(num_envs, torch.uint8)
        self.scratch = z((int(self.L.gvec_pool_collect_scratch_bytes(num_envs)) + 7) // 8, torch.int64)
        a = self.args = CollectArgs()
        a.num_envs, a.obs_floats, a.max_steps_per_episode, a.capacity, a.result_capacity = num_envs, obs_floats, limit, capacity, 0
        for name, tensor in (("ring_state", self.state), ("ring_next_state", self.next_state), ("ring_action", self.action),
                             ("ring_reward", self.reward), ("ring_done", self.done), ("ring_counters", self.counters),
                             ("episode_reward", self.ep_reward), ("episode_length", self.ep_length), ("pool_counters", self.pool_counters),
                             ("scratch", self.scratch), ("needs_reset", self.needs_reset)):
            setattr(a, name, tensor.data_ptr())

    def step(self, x):
        t, a = self.t, self.args
        dev = {k: t.from_numpy(v).cuda() for k, v in x.items()}
        for k, v in dev.items():
            setattr(a, k, v.data_ptr())
        self.before.copy_(self.counters)
        assert self.L.gvec_pool_collect(0, None, C.byref(a)) == 0, self.L.gvec_last_error()
        assert self.L.gvec_nstep_link(0, None, C.byref(a), self.before.data_ptr(), self.succ.data_ptr(), self.last.data_ptr()) == 0, self.L.gvec_last_error()
        t.cuda.synchronize()                       # the step's inputs live until here

    def gather(self, idx, n_step, gamma, succ=True):
        from generalsreinforcementlearning_amd._lib import NstepGatherArgs
        t = self.t
        idx = t.as_tensor(np.asarray(idx, np.int64)).cuda()
        k = len(idx)
        o = dict(state=t.full((k, self.F), 7.0, device="cuda"), next_state=t.full((k, self.F), 7.0, device="cuda"),
                 action=t.full((k,), 7, dtype=t.int64, device="cuda"), ret=t.full((k,), 7.0, dtype=t.float64, device="cuda"),
                 discount=t.full((k,), 7.0, dtype=t.float64, device="cuda"), done=t.full((k,), 7, dtype=t.uint8, device="cuda"),
                 steps=t.full((k,), 7, dtype=t.int32, device="cuda"), last_idx=t.full((k,), 7, dtype=t.int64, device="cuda"))
        a = NstepGatherArgs()
        a.k, a.capacity, a.n_step, a.obs_floats, a.gamma = k, self.cap, n_step, self.F, gamma
        for name, tensor in (("idx", idx), ("ring_state", self.state), ("ring_next_state", self.next_state), ("ring_action", self.action),
                             ("ring_reward", self.reward), ("ring_done", self.done), ("ring_counters", self.counters)) + tuple(o.items()):
            setattr(a, name, tensor.data_ptr())
        a.ring_succ = self.succ.data_ptr() if succ else None
        assert self.L.gvec_nstep_gather(0, None, C.byref(a)) == 0, self.L.gvec_last_error()
        o = {f: v.cpu().numpy() for f, v in o.items()}
        o["done"] = o["done"].astype(bool)
        return o


def _drive(num_envs, capacity, steps, limit, obs_floats, check_every_step=False):
    sc = N.script(num_envs, steps, limit, obs_floats)
    m = N.RingModel(num_envs, capacity, limit, obs_floats)
    ring = _Ring(num_envs, capacity, limit, obs_floats)
    for i, x in enumerate(sc):
        m.step(x)
        ring.step(x)
        if check_every_step:
            assert np.array_equal(ring.succ.cpu().numpy(), m.succ), (capacity, i)
            assert np.array_equal(ring.last.cpu().numpy(), m.last), (capacity, i)
            assert ring.counters.tolist() == [m.cursor, m.size, m.total, 0], (capacity, i)
    return ring, m


@pytest.fixture(scope="module")
def driven():
    """The wrapped ring of the link test on the device with its model, per observation size; built once, never changed."""
    cache = {}

    def get(obs_floats):
        if obs_floats not in cache:
            cache[obs_floats] = _drive(ENVS, 1043, STEPS, LIMIT, obs_floats)
        return cache[obs_floats]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(ENVS, 1043, STEPS, LIMIT), (ENVS, 131, STEPS, LIMIT), (ENVS, 130, STEPS, LIMIT), (5, 23, 30, 4)])
def test_links_match_the_model(case, models):
    n, cap, steps, limit = case
    if n == ENVS:                                  # on the model alone, before the GPU: the inputs exercise every path
        m0 = models[cap][1]
        if cap == 1043:
            assert m0.full_chain_fraction(3) >= 0.40 and m0.ended_by_done >= 50 and m0.ended_by_cut >= 50
        else:
            assert m0.skipped_links >= 1000
    ring, m = _drive(n, cap, steps, limit, 3, check_every_step=True)
    for f in ("state", "next_state", "action", "reward"):
        assert np.array_equal(getattr(ring, f).cpu().numpy()[:m.size], getattr(m, f)[:m.size]), f
    assert np.array_equal(ring.done.cpu().numpy()[:m.size].astype(bool), m.done[:m.size])


def _same(got, want, ctx):
    for f in want:
        a, b = got[f], want[f]
        if a.dtype.kind == "f":                    # bit for bit: floats as their integers
            a, b = a.view(f"u{a.dtype.itemsize}"), b.astype(got[f].dtype).view(f"u{a.dtype.itemsize}")
        assert np.array_equal(a, b), (ctx, f, int((a != b).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("obs_floats", [3, 225, 324, 2025])
def test_gather_is_exact(obs_floats, driven):
    """The batch of 1,045 runs with eight wavefronts per sample; the larger batches below (the same slots repeated) with four,
    two and one - the launcher picks 1 << s, s the smallest with k << s >= 16,384.  225 (5x5) and 2,025 (15x15) floats: rows
    that start on no 16-byte boundary; the out-of-range indices stay in every batch."""
    ring, m = driven(obs_floats)
    idx = np.concatenate([np.arange(m.size), [-1, m.size]])
    for n_step in (1, 2, 3, 5):
        for gamma in (0.99, 1.0, 0.5):
            got = ring.gather(idx, n_step, gamma)
            _same(got, m.gather(idx, n_step, gamma, "tags"), (obs_floats, n_step, gamma))
            for f, zero in (("steps", 0), ("ret", 0.0), ("discount", 0.0), ("done", False), ("action", -1), ("last_idx", -1)):
                assert (got[f][-2:] == zero).all(), f
            assert not got["state"][-2:].any() and not got["next_state"][-2:].any()
            steps = got["steps"][:-2]
            assert steps.max() == n_step and set(steps.tolist()) == set(range(1, n_step + 1))
    want = m.gather(idx, 3, 0.99, "tags")
    for k in (5000, 10000, 17000):                                     # four, two, one wavefront(s) per sample
        rep = np.resize(np.arange(len(idx)), k)
        got = ring.gather(idx[rep], 3, 0.99)
        _same(got, {f: v[rep] for f, v in want.items()}, (obs_floats, "batch", k))
    one = ring.gather(idx[:-2], 1, 0.99, succ=False)                   # n_step 1 needs no links: ring[idx] field for field
    for f, slab in (("state", ring.state), ("next_state", ring.next_state), ("action", ring.action), ("ret", ring.reward)):
        assert np.array_equal(one[f], slab.cpu().numpy()[:m.size]), f
    assert np.array_equal(one["done"], ring.done.cpu().numpy()[:m.size].astype(bool))
    assert (one["discount"] == 0.99).all() and (one["steps"] == 1).all() and np.array_equal(one["last_idx"], idx[:-2])


def _check_chains(state, next_state, steps, done, n_step, limit, newest, ctx=""):
    """Property 3 on a batch's tags alone: one (worker, episode), consecutive t, short only for a reason.  `newest`:
    {worker: (episode, t)} of each worker's newest row."""
    w0, e0, t0 = N.untag(state[:, 0])
    w1, e1, t1 = N.untag(next_state[:, 0])
    assert (steps >= 1).all() and (steps <= n_step).all(), ctx
    assert np.array_equal(w0, w1) and np.array_equal(e0, e1), ctx       # the chain never leaves its worker's episode
    assert np.array_equal(t1, t0 + steps), ctx                         # next_state is that of row t0 + steps - 1: t advanced by steps
    for j in np.flatnonzero(steps < n_step):
        tl = t1[j] - 1
        assert done[j] or tl + 1 >= limit or newest.get(int(w0[j])) == (int(e0[j]), int(tl)), (ctx, j, w0[j], e0[j], tl)


def _newest(ring_state, seq_order):
    """{worker: (episode, t)} of the newest row of every worker; seq_order: held slots from oldest to newest."""
    w, e, t = N.untag(ring_state[seq_order, 0])
    return {int(w[i]): (int(e[i]), int(t[i])) for i in range(len(seq_order))}


@pytest.mark.gpu
@pytest.mark.parametrize("n_step", [2, 3, 5])
def test_no_chain_crosses_a_boundary(n_step, driven):
    ring, m = driven(3)
    size, cursor = int(ring.counters[1]), int(ring.counters[0])
    idx = np.arange(size)
    got = ring.gather(idx, n_step, 0.99)
    state, succ = ring.state.cpu().numpy(), ring.succ.cpu().numpy()
    order = (cursor + np.arange(size)) % size                           # a full ring: the oldest row sits at the cursor
    _check_chains(got["state"], got["next_state"], got["steps"], got["done"], n_step, LIMIT, _newest(state, order), n_step)
    for j in idx:                                                       # every row visited, not only the two ends
        w, e, t = N.untag(state[j, 0])
        cur = j
        for i in range(1, got["steps"][j]):
            cur = succ[cur]
            assert N.untag(state[cur, 0]) == (w, e, t + i), (j, i)
        assert cur == got["last_idx"][j]


def _random_valid(states, masks, workers, generator):
    import torch
    return (masks * torch.rand(masks.shape, device=masks.device, generator=generator)).argmax(1)      # every worker explores for itself


def _pool(buf, B=64, board=6, seed=2, steps=5):
    """A pool whose observations identify the worker as far as an env's can: 4,096 boards dealt by hash (a deal is shared with
    another of B workers with probability under B / 4096) and a policy that draws a uniform valid action per worker."""
    from generalsreinforcementlearning_amd.env_pool import ParallelVecEnvPool
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    return ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=board, board_height=board, max_players=2, seed=seed, board_pool=4096,
                                                         device_outputs=True),
                              _random_valid, buf, max_steps_per_episode=steps, batched_actions=True, seed=seed)


def _unique_share(rows32):
    """The share of rows (int32 views of observations) that no other row equals bit for bit."""
    import torch
    _, inv, cnt = torch.unique(rows32, dim=0, return_inverse=True, return_counts=True)
    return float((cnt[inv] == 1).double().mean())


@pytest.mark.gpu
@pytest.mark.parametrize("prioritized", [False, True])
def test_pool_integration(prioritized):
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    cls = PrioritizedDeviceReplayBuffer if prioritized else DeviceReplayBuffer
    gamma = 0.97
    buf = cls(1000, n_step=3, gamma=gamma)
    pool = _pool(buf)
    pool.collect(25)
    torch.cuda.synchronize()
    assert buf.total_pushed > 1000 == len(buf)                          # the ring wrapped
    succ = buf.ring_succ.cpu()
    linked = torch.nonzero(succ >= 0).flatten()
    assert 300 < len(linked) and int(succ.max()) < 1000
    s, ns = buf.state.cpu().view(1000, -1).view(torch.int32), buf.next_state.cpu().view(1000, -1).view(torch.int32)
    assert torch.equal(s[succ[linked]], ns[linked])                     # an env's next observation IS its next state
    share = _unique_share(s)                                            # ... and names its worker where no other row equals it
    print(f"NSTEP-MEASURE pool unique observations {share:.3f}")
    assert share > 0.5
    assert (succ[buf.done.cpu()] == -1).all()
    out = buf.sample_nstep(256)
    assert len(out) == 7
    if prioritized:
        out9 = buf.sample_nstep_prioritized(256)
        assert len(out9) == 9 and out9[7].dtype == torch.int64 and out9[8].dtype == torch.float32 and out9[7].shape == out9[8].shape == (256,)
        assert torch.equal(out9[0], buf.state[out9[7]]) and torch.equal(out9[1], buf.action[out9[7]])
        R.check_invariant(buf, "n-step pool")
        outs = [out, out9[:7]]
    else:
        outs = [out, buf.gather_nstep(torch.arange(1000))]
    for states, actions, returns, next_states, dones, discounts, steps in outs:
        k = len(actions)
        assert states.shape == next_states.shape == (k,) + buf.obs_shape and states.dtype == torch.float32 and states.is_cuda
        assert actions.dtype == torch.int64 and returns.dtype == discounts.dtype == torch.float64 and dones.dtype == torch.bool
        assert steps.dtype == torch.int32 and int(steps.min()) >= 1 and int(steps.max()) == 3
        want = np.array([[np.float64(gamma), np.float64(gamma) * gamma, np.float64(gamma) * gamma * gamma][i - 1] for i in steps.tolist()])
        assert np.array_equal(discounts.cpu().numpy(), want)
    # sample_arrays stays one-step on an n-step buffer
    buf.manual_seed(3)
    five = buf.sample_arrays(64)
    assert len(five) == 5
    pool._env.close()


@pytest.mark.gpu
def test_n_step_one_changes_nothing():
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer
    rings = []
    for kw in ({}, {"n_step": 1}, {"n_step": 3}):
        buf = DeviceReplayBuffer(1000, **kw)
        pool = _pool(buf)
        pool.collect(25)
        torch.cuda.synchronize()
        rings.append((buf, pool._dc))
        pool._env.close()
    (a, _), (b, dc), (c, dc3) = rings
    assert b.ring_succ is None and b._before is None and dc.nstep_last is None and dc3.nstep_last is not None
    for other in (b, c):                                               # the links ride beside the ring: its rows do not change
        assert torch.equal(a.counters, other.counters)
        for f in ("state", "next_state", "action", "reward", "done"):
            assert torch.equal(getattr(a, f).view(torch.uint8), getattr(other, f).view(torch.uint8)), f
    s, act, ret, ns, d, disc, steps = b.gather_nstep(torch.arange(1000))
    assert torch.equal(s, b.state) and torch.equal(act, b.action) and torch.equal(ret, b.reward) and torch.equal(ns, b.next_state)
    assert torch.equal(d, b.done) and (disc == 0.99).all() and (steps == 1).all()


@pytest.mark.gpu
def test_push_batch_rows_are_chains_of_one():
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        buf = cls(100, n_step=3, gamma=0.9).allocate((3,))
        buf.ring_succ[:] = torch.arange(100, device=buf.device).roll(-1)   # stale links everywhere: push_batch must clear its rows'
        k = 130                                                            # wraps
        buf.push_batch(torch.rand(k, 3), torch.arange(k), torch.arange(k).double(), torch.rand(k, 3), torch.zeros(k, dtype=torch.bool))
        assert (buf.ring_succ == -1).all()
        s, a, ret, ns, d, disc, steps = buf.gather_nstep(torch.arange(100))
        assert (steps == 1).all() and torch.equal(ret, buf.reward) and (disc == 0.9).all() and torch.equal(ns, buf.next_state)
        s, a, ret, ns, d, disc, steps = buf.sample_nstep(32)
        assert (steps == 1).all() and torch.equal(ret, a.double())


@pytest.mark.gpu
def test_sampling_while_a_pool_thread_collects():
    """A collector thread appends and links while the main thread draws: every batch is made of whole chains.  A real env's
    observations carry no tag; the ring is large enough not to wrap, so a slot IS its row's sequence number, and a chain is
    checked by what makes it one: every hop leads to the row whose state is the predecessor's next_state, nothing follows a
    done row, and a chain is short only where its last row is done, has no successor to this day, or was the worker's newest
    at the time (its successor was appended after the draw).  This is weaker than property 3 on tags in one way that cannot
    be helped here: "no successor to this day" reads the links themselves, so a link the kernel wrongly DROPPED would pass -
    dropped and misplaced links are what the synthetic, tagged tests above are for (test_links_match_the_model compares every
    link with the model after every step).  The hop check identifies the worker as far as observations do: most rows are
    unique in the ring (asserted below)."""
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer
    limit, n_step, gamma = 6, 3, 0.9
    buf = DeviceReplayBuffer(1 << 21, n_step=n_step, gamma=gamma)
    pool = _pool(buf, B=512, steps=limit)
    pool.start()
    t0 = time.time()
    while pool.total_env_steps < 4 * 512 and time.time() - t0 < 60:
        time.sleep(0.01)
    draws = []
    for i in range(200):
        out = buf.sample_nstep(128)
        assert len(out) == 7
        with buf._guard:                                                # the same, with the indices and the counters of the moment
            idx = buf.sample_indices(128)
            o = buf._gather_nstep(idx)
            draws.append((idx, o, buf.counters.clone()))
    pool.stop(join_timeout=10.0)
    torch.cuda.synchronize()
    assert buf.total_pushed < buf.capacity and len(draws) == 200
    succ, done, cap = buf.ring_succ, buf.done, buf.capacity
    s32, n32 = buf.state.view(cap, -1).view(torch.int32), buf.next_state.view(cap, -1).view(torch.int32)
    for idx, o, counters in draws:
        steps, last, pushed = o["steps"], o["last_idx"], int(counters[2])
        assert int(steps.min()) >= 1 and int(steps.max()) <= n_step and int(idx.max()) < pushed
        assert torch.equal(o["state"], buf.state[idx]) and torch.equal(o["action"], buf.action[idx])
        assert torch.equal(o["next_state"], buf.next_state[last]) and torch.equal(o["done"], done[last])
        cur, ret, disc = idx.clone(), buf.reward[idx].clone(), torch.ones_like(buf.reward[idx])
        for i in range(1, n_step):                                      # the walk over today's links: a link, once set, stays
            go = steps > i
            assert not bool(done[cur][go].any())                        # nothing follows a done row
            nxt = torch.where(go, succ[cur], cur)
            assert int(nxt.min()) >= 0 and int(nxt.max()) < pushed
            assert torch.equal(s32[nxt[go]], n32[cur[go]])              # the same env's next step
            cur = nxt
            disc = torch.where(go, disc * gamma, disc)
            ret = torch.where(go, ret + disc * buf.reward[cur], ret)
        assert torch.equal(cur, last) and torch.equal(ret, o["ret"]) and torch.equal(disc * gamma, o["discount"])
        short = steps < n_step
        assert bool((~short | done[last] | (succ[last] < 0) | (succ[last] >= pushed)).all())
    linked = torch.nonzero(succ[:len(buf)] >= 0).flatten()
    assert len(linked) > 512 and torch.equal(s32[succ[linked]], n32[linked])
    share = _unique_share(s32[:min(len(buf), 5000)])                    # the first ~10 steps: ~1,000 deals out of 4,096 boards (later, boards recur)
    print(f"NSTEP-MEASURE live pool unique observations {share:.3f}")
    assert share > 0.5
