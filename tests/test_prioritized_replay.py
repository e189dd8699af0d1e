"""Prioritized experience replay on the device replay ring (gvec_per_*, PrioritizedDeviceReplayBuffer)
against the float64 model of _per_reference.py.  L = tree levels above the leaves, eps = 2^-24."""
import ctypes as C
import os
import re
import threading
import time

import numpy as np
import pytest

import _per_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = ["gvec_per_tree_bytes", "gvec_per_tree_layout", "gvec_per_init", "gvec_per_push", "gvec_per_update", "gvec_per_sample"]

# Largest relative error of a leaf (|td| + eps) ** alpha against float64 numpy over the cases of test_leaves_* (alpha in
# {0.4, 0.6, 1.0}, |td| over 1e-4 .. 1e3), measured on an MI355X: 3.7e-7 (1.9e-7 / 3.7e-7 / 1.7e-7 for the three alphas: the float32 sum, then powf).  The
# tolerance is 4 x that.
LEAF_MEASURED, LEAF_TOL = 3.7e-7, 1.5e-6
# Largest relative error of a weight against the float64 model on the read-back leaves over the cases of test_weights_*,
# measured: 1.9e-7 (0 / 1.9e-7 / 1.4e-7 for beta 0 / 0.4 / 1: a float32 division, then powf).  The tolerance is 4 x that.
WEIGHT_MEASURED, WEIGHT_TOL = 1.9e-7, 7.7e-7


# ---- without a GPU ----------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_documented():
    from generalsreinforcementlearning_amd import _lib
    import generalsreinforcementlearning_amd as g
    hdr = open(os.path.join(ROOT, "include", "generals_vec.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = g.load()
    for name in PER:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in doc, name
    assert L.gvec_abi_version() == 2
    assert g.PrioritizedDeviceReplayBuffer is not None


def test_layout_query():
    import generalsreinforcementlearning_amd as g
    L = g.load()
    out = (C.c_int64 * 10)()
    for cap, levels in ((1, 1), (64, 1), (65, 2), (1000, 2), (4096, 2), (4097, 3), (65536, 3), (1 << 20, 4), (1 << 24, 4), ((1 << 24) + 1, 5)):
        assert L.gvec_per_tree_layout(cap, out) == 0
        assert out[0] == levels, (cap, list(out))
        n, at = cap, 64
        for l in range(levels + 1):
            assert out[2 + l] == at
            at += (n + 63) // 64 * 64
            n = (n + 63) // 64
        assert n == 1 and out[1] == at and L.gvec_per_tree_bytes(cap) == 4 * at
    assert L.gvec_per_tree_bytes(0) == 0 and L.gvec_per_tree_layout(0, out) == -1 and L.gvec_per_tree_layout(8, None) == -1


def test_argument_checks_need_no_device():
    import generalsreinforcementlearning_amd as g
    L = g.load()
    t, p, bad = C.c_void_p(4096), C.c_void_p(4096), C.c_void_p(4096 + 64)
    inv = lambda rc, word: rc == -1 and word in L.gvec_last_error()
    assert inv(L.gvec_per_init(0, None, None, 100), b"NULL")
    assert inv(L.gvec_per_init(0, None, t, 0), b"capacity")
    assert inv(L.gvec_per_init(0, None, bad, 100), b"aligned")
    assert inv(L.gvec_per_push(0, None, None, 100, p, p, 10), b"NULL")
    assert inv(L.gvec_per_push(0, None, t, 0, p, p, 10), b"capacity")
    assert inv(L.gvec_per_push(0, None, bad, 100, p, p, 10), b"aligned")
    assert inv(L.gvec_per_push(0, None, t, 100, None, p, 10), b"NULL")
    assert inv(L.gvec_per_push(0, None, t, 100, p, p, 0), b"max_count")
    assert inv(L.gvec_per_update(0, None, None, 100, p, p, 4, 0.6, 1e-6), b"NULL")
    assert inv(L.gvec_per_update(0, None, t, -5, p, p, 4, 0.6, 1e-6), b"capacity")
    assert inv(L.gvec_per_update(0, None, bad, 100, p, p, 4, 0.6, 1e-6), b"aligned")
    assert inv(L.gvec_per_update(0, None, t, 100, p, p, -1, 0.6, 1e-6), b"n -1")
    assert inv(L.gvec_per_update(0, None, t, 100, p, p, 4, -0.1, 1e-6), b"alpha")
    assert inv(L.gvec_per_update(0, None, t, 100, p, p, 4, 0.6, 0.0), b"eps")
    assert inv(L.gvec_per_update(0, None, t, 100, p, p, 4, 0.6, -1.0), b"eps")
    assert inv(L.gvec_per_update(0, None, t, 100, None, p, 4, 0.6, 1e-6), b"NULL")
    assert L.gvec_per_update(0, None, t, 100, None, None, 0, 0.6, 1e-6) == 0            # n == 0: a no-op, no device
    assert inv(L.gvec_per_sample(0, None, None, 100, p, 4, 0.4, None, 0, p, p), b"NULL")
    assert inv(L.gvec_per_sample(0, None, t, 0, p, 4, 0.4, None, 0, p, p), b"capacity")
    assert inv(L.gvec_per_sample(0, None, bad, 100, p, 4, 0.4, None, 0, p, p), b"aligned")
    assert inv(L.gvec_per_sample(0, None, t, 100, p, 0, 0.4, None, 0, p, p), b"k 0")
    assert inv(L.gvec_per_sample(0, None, t, 100, p, 4, -0.5, None, 0, p, p), b"beta")
    assert inv(L.gvec_per_sample(0, None, t, 100, p, 4, 0.4, None, 0, None, p), b"NULL")


# ---- on the GPU ----------------------------------------------------------------------------------------------------
def _buffer(capacity, size=None, **kw):
    """A prioritized buffer over a ring of one-float observations that says it holds `size` transitions."""
    import torch
    from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
    buf = PrioritizedDeviceReplayBuffer(capacity, **kw).allocate((1,))
    size = capacity if size is None else size
    buf.counters[:3] = torch.tensor([size % capacity, size, size], dtype=torch.int64)
    return buf


def _with_leaves(leaves, size=None):
    """A fresh tree whose leaves are `leaves` (float32; zeros stay the zeros of gvec_per_init), through gvec_per_update."""
    import torch
    leaves = np.asarray(leaves, np.float32)
    buf = _buffer(len(leaves), size, alpha=1.0, eps=1e-30)
    nz = np.flatnonzero(leaves)
    buf.update_priorities(torch.from_numpy(nz), torch.from_numpy(leaves[nz]))
    got, _ = R.check_invariant(buf, "leaves set")
    assert np.array_equal(got == 0, leaves == 0)                  # the zeros are exact; pow(x, 1) is within the leaf tolerance
    assert (np.abs(got[nz] - leaves[nz]) <= LEAF_TOL * leaves[nz]).all()
    return buf, got


def _first_valid(states, masks, workers, generator):
    return masks.to(dtype=__import__("torch").uint8).argmax(1)


def _pool(buf, B=64, board=6, seed=2, steps=3):
    from generalsreinforcementlearning_amd.env_pool import ParallelVecEnvPool
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    return ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=board, board_height=board, max_players=2, seed=seed, board_pool=8,
                                                         device_outputs=True),
                              _first_valid, buf, max_steps_per_episode=steps, batched_actions=True, seed=seed)


@pytest.mark.gpu
def test_tree_invariant_after_init_wrapping_push_and_duplicate_update():
    import torch
    from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
    cap = 1000
    buf = PrioritizedDeviceReplayBuffer(cap).allocate((3,))
    leaves, top = R.check_invariant(buf, "init")
    assert not leaves.any() and top == 1.0
    mk = lambda k: (torch.rand(k, 3), torch.arange(k), torch.rand(k).double(), torch.rand(k, 3), torch.zeros(k, dtype=torch.bool))
    buf.push_batch(*mk(700))
    leaves, top = R.check_invariant(buf, "push")
    assert (leaves[:700] == 1.0).all() and not leaves[700:].any() and top == 1.0 and len(buf) == 700
    idx = torch.tensor([5, 5, 5, 699, 64, 63, 5, 128])
    td = torch.tensor([2.0, 3.0, 4.0, 0.5, 7.0, 0.25, 5.0, 1.0])
    buf.update_priorities(idx, td)
    leaves, top = R.check_invariant(buf, "duplicates")
    want = R.leaf_value(td.numpy(), buf.alpha, buf.eps)
    assert any(abs(leaves[5] - want[i]) <= LEAF_TOL * want[i] for i in (0, 1, 2, 6))          # any one of the supplied values
    for i in (3, 4, 5, 7):
        assert abs(leaves[idx[i]] - want[i]) <= LEAF_TOL * want[i]
    assert top == np.float32(leaves.max()) and top >= np.float32(want[4]) * (1 - LEAF_TOL)
    buf.push_batch(*mk(450))                                  # wraps: slots 700..999 and 0..149 are new
    leaves, top2 = R.check_invariant(buf, "wrapping push")
    assert top2 == top and (leaves[700:] == top).all() and (leaves[:150] == top).all() and len(buf) == cap
    assert abs(leaves[699] - want[3]) <= LEAF_TOL * want[3] and leaves[150] == 1.0
    buf.push_batch(*mk(2500))                                 # longer than the ring: every slot is new
    leaves, _ = R.check_invariant(buf, "over-long push")
    assert (leaves == top).all()
    # out-of-range indices and non-finite errors are skipped and counted on the device
    buf.update_priorities(torch.tensor([-1, cap, 3, 4]), torch.tensor([1.0, 1.0, float("nan"), 0.5]))
    leaves, _ = R.check_invariant(buf, "rejects")
    assert buf.rejected_updates == 3 and leaves[3] == top and abs(leaves[4] - R.leaf_value(0.5, buf.alpha, buf.eps)) < 1e-6


@pytest.mark.gpu
def test_tree_invariant_over_interleaved_collect_and_update_rounds():
    import torch
    from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
    buf = PrioritizedDeviceReplayBuffer(1000, alpha=0.6)
    pool = _pool(buf)
    g = torch.Generator().manual_seed(5)
    ever, pushed = np.float32(1.0), 0                         # the largest leaf ever written (the maximum starts at 1.0)
    for rnd in range(50):
        pool.collect(1 + rnd % 3)
        s, a, r, ns, d, idx, w = buf.sample_prioritized(32)
        idx = idx.unique()                                    # distinct slots: every value written is there to be read back
        td = (torch.rand(len(idx), generator=g) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g))).float()
        buf.update_priorities(idx, td)
        leaves, top = R.check_invariant(buf, f"round {rnd}")
        size = len(buf)
        assert size > pushed or size == 1000
        pushed = size
        assert (leaves[:size] > 0).all() and not leaves[size:].any()
        ever = max(ever, np.float32(leaves.max()))
        assert np.float32(top) == ever, (rnd, top, ever)      # exactly the largest leaf ever written
    # rows the pool appends carry the maximum
    before, pushed = int(buf.counters[0]), buf.total_pushed
    pool.collect(2)                                           # (a step on which every worker re-deals appends nothing)
    leaves, top = R.check_invariant(buf, "after the last collect")
    n = buf.total_pushed - pushed
    assert n > 0 and all(leaves[(before + i) % 1000] == top for i in range(n))
    pool._env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.4, 0.6, 1.0])
def test_leaves_match_float64_pow(alpha):
    import torch
    cap, eps = 65536, 1e-6
    buf = _buffer(cap, alpha=alpha, eps=eps)
    rng = np.random.default_rng(7)
    td = (10.0 ** rng.uniform(-4, 3, cap)).astype(np.float32) * rng.choice([-1.0, 1.0], cap).astype(np.float32)
    td[:8] = [1e-4, -1e-4, 1e3, -1e3, 1.0, -1.0, 0.5, 2.0]
    idx = rng.permutation(cap)
    buf.update_priorities(torch.from_numpy(idx), torch.from_numpy(td))
    leaves, top = R.check_invariant(buf, f"alpha {alpha}")
    want = R.leaf_value(td, alpha, eps)
    err = np.abs(leaves[idx] - want) / want
    print(f"PER-MEASURE leaf alpha={alpha} max_rel_err={err.max():.3e}")
    assert err.max() <= LEAF_TOL, err.max()
    assert top == max(1.0, leaves.max())
    # rows pushed afterwards carry the maximum
    k = 100
    buf.push_batch(torch.zeros(k, 1), torch.zeros(k, dtype=torch.int64), torch.zeros(k, dtype=torch.float64), torch.zeros(k, 1),
                   torch.zeros(k, dtype=torch.bool))
    after, top2 = R.check_invariant(buf, "push after update")
    assert top2 == top and (after[:k] == top).all() and np.array_equal(after[k:], leaves[k:])


def _leaf_cases(cap, rng):
    base = (10.0 ** rng.uniform(-1, 1, cap)).astype(np.float32)
    full = base.copy()
    part = base.copy()
    part[cap * 3 // 5:] = 0                                                     # a partly filled ring
    runs = base.copy()
    for lo in rng.integers(0, cap, 12):
        runs[lo:lo + int(rng.integers(1, max(2, cap // 10)))] = 0               # long runs of zero leaves
    runs[0], runs[-1] = 0, 0
    spike = np.ones(cap, np.float32)
    spike[cap // 3] = 1e6                                                       # one leaf 10^6 times the others
    return {"full": (full, cap), "part": (part, cap * 3 // 5), "runs": (runs, cap), "spike": (spike, cap)}


def _check_draws(buf, leaves, size, k, u, ctx):
    import torch
    s, a, r, ns, d, idx, w = buf.sample_prioritized(k, u=torch.from_numpy(np.asarray(u, np.float64)))
    idx = idx.cpu().numpy()
    F = R.prefix(leaves)
    t = R.targets(k, u, F[-1])
    s_ = R.slack(buf.tree_levels, F[-1])
    assert (idx >= 0).all() and (idx < size).all(), ctx
    assert (leaves[idx] > 0).all(), ctx                                         # exact: a zero leaf is never drawn
    lo_ok, hi_ok = F[idx] - s_ <= t, t <= F[idx + 1] + s_
    assert lo_ok.all() and hi_ok.all(), f"{ctx}: {int((~lo_ok).sum())} below, {int((~hi_ok).sum())} above their bracket"
    return idx, w.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1000, 65536, 1 << 20, 1 << 24])
def test_draw_is_the_bracket(cap):
    rng = np.random.default_rng(cap)
    for name, (leaves32, size) in _leaf_cases(cap, rng).items():
        if cap == 1 << 24 and name not in ("runs", "spike"):
            continue                                                            # the 16 M tree: the two hardest shapes (a minute each)
        buf, leaves = _with_leaves(leaves32, size)
        for k in (1, 7, 256, 32768):
            if k > size:
                continue
            grid = np.linspace(0.0, 1.0, k, endpoint=False)
            _check_draws(buf, leaves, size, k, grid, f"{cap} {name} k={k} grid")
            _check_draws(buf, leaves, size, k, np.zeros(k), f"{cap} {name} k={k} u=0")
            _check_draws(buf, leaves, size, k, np.full(k, 1.0 - 2.0 ** -53), f"{cap} {name} k={k} u->1")
            _check_draws(buf, leaves, size, k, rng.random(k), f"{cap} {name} k={k} random")
        del buf


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [1.0, 0.0])
def test_frequencies_with_fixed_u(alpha):
    import torch
    n, k = 4096, 1 << 20
    rng = np.random.default_rng(3)
    pri = (10.0 ** rng.uniform(-1.5, 1.5, n)).astype(np.float32)                # three decades
    buf = _buffer(n, alpha=alpha, eps=1e-30, beta=0.5)
    buf.update_priorities(torch.arange(n), torch.from_numpy(pri))
    leaves, _ = R.check_invariant(buf, "frequencies")
    if alpha == 0.0:
        assert (leaves == 1.0).all()
    u = np.full(k, 0.5)
    with buf._guard:      # gvec_per_sample itself: more draws than slots (sample_prioritized keeps the uniform buffer's batch <= len contract)
        idx, w = buf._draw(k, None, torch.from_numpy(u))
    count = np.bincount(idx.cpu().numpy(), minlength=n)
    total = leaves.sum()
    bound = 2 * (1 + k * R.slack(buf.tree_levels, total) / total)
    dev = np.abs(count - k * leaves / total)
    print(f"PER-MEASURE frequencies alpha={alpha} max_dev={dev.max():.2f} bound={bound:.2f}")
    assert dev.max() <= bound, (dev.max(), bound)
    if alpha == 0.0:
        assert (w.cpu().numpy() == 1.0).all() and count.min() == count.max() == k // n


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_weights_match_the_model(beta):
    import torch
    cap, size, k = 65536, 50000, 8192
    rng = np.random.default_rng(11)
    leaves32 = (10.0 ** rng.uniform(-2, 2, cap)).astype(np.float32)
    leaves32[size:] = 0
    buf, leaves = _with_leaves(leaves32, size)
    s, a, r, ns, d, idx, w = buf.sample_prioritized(k, beta=beta, u=torch.from_numpy(rng.random(k)))
    idx, w = idx.cpu().numpy(), w.cpu().numpy().astype(np.float64)
    want = R.weights(leaves, idx, size, beta)
    err = np.abs(w - want) / want
    print(f"PER-MEASURE weight beta={beta} max_rel_err={err.max():.3e}")
    assert err.max() <= WEIGHT_TOL, err.max()
    assert w.max() == 1.0
    if beta == 0.0:
        assert (w == 1.0).all()


@pytest.mark.gpu
def test_contract_seed_and_returns():
    import torch
    from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
    with pytest.raises(ValueError):
        PrioritizedDeviceReplayBuffer(0)
    with pytest.raises(ValueError):
        PrioritizedDeviceReplayBuffer(10, alpha=-1)

    def fresh():
        buf = PrioritizedDeviceReplayBuffer(5000, alpha=0.6).allocate((2, 3))
        g = torch.Generator().manual_seed(1)
        k = 3000
        buf.push_batch(torch.rand(k, 2, 3, generator=g), torch.arange(k), torch.arange(k).double() / 7, torch.rand(k, 2, 3, generator=g), torch.arange(k) % 2 == 0)
        buf.update_priorities(torch.arange(k), torch.rand(k, generator=g) * 5)
        return buf
    empty = PrioritizedDeviceReplayBuffer(100)
    with pytest.raises(ValueError):
        empty.sample_prioritized(1)
    a, b = fresh(), fresh()
    with pytest.raises(ValueError):
        a.sample_prioritized(3001)
    with pytest.raises(ValueError):
        a.sample_arrays(3001)
    a.manual_seed(11)
    b.manual_seed(11)
    ia = [a.sample_prioritized(256)[5] for _ in range(3)]
    ib = [b.sample_prioritized(256)[5] for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(ia, ib)) and not torch.equal(ia[0], ia[1])
    a.manual_seed(11)
    assert torch.equal(a.sample_prioritized(256)[5], ia[0])                      # the sequence restarts
    a.manual_seed(12)
    assert not torch.equal(a.sample_prioritized(256)[5], ia[0])
    s, act, r, ns, d, idx, w = a.sample_prioritized(200)
    assert s.is_cuda and s.shape == (200, 2, 3) and idx.dtype == torch.int64 and w.dtype == torch.float32 and int(idx.max()) < 3000
    assert torch.equal(s, a.state[idx]) and torch.equal(act, a.action[idx]) and torch.equal(r, a.reward[idx])
    assert torch.equal(ns, a.next_state[idx]) and torch.equal(d, a.done[idx]) and torch.equal(act, idx)
    assert float(w.max()) == 1.0 and float(w.min()) > 0
    # stratified: draw j lies in the j-th of 200 equal shares of the total priority, so the indices ascend
    assert bool((idx[1:] >= idx[:-1]).all())
    with pytest.raises(ValueError):
        a.sample_indices(3001)
    with pytest.raises(ValueError):
        empty.sample_indices(1)
    assert int(a.sample_indices(64).max()) < 3000
    five = a.sample_arrays(64)
    assert len(five) == 5 and five[0].shape == (64, 2, 3)
    tuples = a.sample(5)
    assert len(tuples) == 5 and tuples[0][0].shape == (2, 3) and isinstance(tuples[0][1], int) and isinstance(tuples[0][4], bool)


@pytest.mark.gpu
def test_draws_while_a_pool_thread_collects_are_whole_transitions():
    import torch
    from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
    buf = PrioritizedDeviceReplayBuffer(1 << 21, alpha=0.6)          # large enough not to wrap: a drawn row stays checkable
    pool = _pool(buf, B=512, board=6, steps=25)
    pool.start()
    t0 = time.time()
    while pool.total_env_steps < 4 * 512 and time.time() - t0 < 60:
        time.sleep(0.01)
    draws = []
    for i in range(40):
        out = buf.sample_prioritized(256)
        buf.update_priorities(out[5], torch.rand(256, device=out[5].device) * 3)
        draws.append(out)
    pool.stop(join_timeout=10.0)
    assert buf.total_pushed < buf.capacity and len(draws) == 40
    for s, a, r, ns, d, idx, w in draws:
        assert int(idx.min()) >= 0 and int(idx.max()) < len(buf)
        assert torch.equal(s, buf.state[idx]) and torch.equal(a, buf.action[idx]) and torch.equal(r, buf.reward[idx])
        assert torch.equal(ns, buf.next_state[idx]) and torch.equal(d, buf.done[idx])
        assert float(w.max()) == 1.0 and float(w.min()) > 0
    leaves, top = R.check_invariant(buf, "after the thread")
    size = len(buf)
    assert (leaves[:size] > 0).all() and not leaves[size:].any() and buf.rejected_updates == 0


@pytest.mark.gpu
def test_pool_fills_the_prioritized_ring_like_the_uniform_one():
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    rings = []
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        buf = cls(1000)
        pool = _pool(buf, B=64, steps=3)
        pool.collect(23)                                       # wraps the ring
        torch.cuda.synchronize()
        rings.append((buf, pool.pop_episode_results()))
        pool._env.close()
    (u, ru), (p, rp) = rings
    assert torch.equal(u.counters, p.counters) and ru == rp and len(u) == 1000
    for f in ("state", "next_state", "action", "reward", "done"):
        assert torch.equal(getattr(u, f).view(torch.uint8), getattr(p, f).view(torch.uint8)), f
    leaves, top = R.check_invariant(p, "drop-in")
    assert (leaves == 1.0).all() and top == 1.0


@pytest.mark.gpu
def test_example_runs_prioritized():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_dqn_resident", os.path.join(ROOT, "examples", "train_dqn_resident.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(["--prioritized", "--num-envs", "256", "--board", "8", "--buffer-size", "20000", "--batch-size", "128", "--updates", "6",
                  "--warmup-steps", "4", "--max-steps-per-episode", "30"])
    assert out["updates"] == 6 and all(np.isfinite(x) for x in out["loss"]) and out["ring_fill"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("warm_up_draws", [1, 2, 3])
def test_weights_after_a_reseed_of_a_used_buffer(warm_up_draws):
    """Restarting the seed's sequence (manual_seed, or zeroing the header's draw counter) must not leave the last batch's
    smallest leaf behind: the weights of the next batch are the model's, their largest 1."""
    import torch
    cap, k = 4096, 256
    buf = _buffer(cap, alpha=1.0, eps=1e-30, beta=0.4)
    buf.update_priorities(torch.arange(cap), torch.full((cap,), 1e-3))
    for _ in range(warm_up_draws):
        buf.sample_prioritized(k)                              # batches whose smallest leaf is 1e-3
    buf.update_priorities(torch.arange(cap), 1.0 + torch.arange(cap) / cap)   # every priority raised
    buf.manual_seed(5)
    leaves, _ = R.check_invariant(buf, "reseed")
    for call in range(3):
        idx, w = buf.sample_prioritized(k)[5:]
        idx, w = idx.cpu().numpy(), w.cpu().numpy().astype(np.float64)
        want = R.weights(leaves, idx, cap, 0.4)
        assert w.max() == 1.0 and (np.abs(w - want) <= WEIGHT_TOL * want).all(), (warm_up_draws, call, w.max())


@pytest.mark.gpu
def test_non_finite_errors_are_rejected_at_alpha_zero_and_push_batch_is_one_step():
    import torch
    buf = _buffer(1000, alpha=0.0, eps=1e-6)
    buf.update_priorities(torch.tensor([1, 2, 3, 4]), torch.tensor([float("nan"), float("inf"), -float("inf"), 2.0]))
    leaves, top = R.check_invariant(buf, "alpha 0")
    assert buf.rejected_updates == 3 and not leaves[1:4].any() and leaves[4] == 1.0 and top == 1.0
    # push_batch: only the rows pushed get the maximum, an earlier update next to them stays
    buf = _buffer(1000, size=0, alpha=1.0, eps=1e-30)
    mk = lambda k: (torch.rand(k, 1), torch.arange(k), torch.rand(k).double(), torch.rand(k, 1), torch.zeros(k, dtype=torch.bool))
    buf.push_batch(*mk(100))
    buf.update_priorities(torch.arange(100), torch.full((100,), 0.25))
    buf.push_batch(*mk(10))
    leaves, top = R.check_invariant(buf, "push after update")
    assert (leaves[:100] == 0.25).all() and (leaves[100:110] == 1.0).all() and not leaves[110:].any() and len(buf) == 110
