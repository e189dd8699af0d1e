"""The idioms the learner-side kernel units share (gvec_waves.hpp, gvec_rows.hpp), through the public calls that use them:
the row movers at every pair of source and destination alignments and at the row sizes where head, body and tail are empty,
one quad or barely more, and the one-workgroup scan at the item counts where a thread's run is empty, one item, or two.
Everything is compared bit for bit with numpy indexing; guard values around every output must survive."""
import ctypes as C

import numpy as np
import pytest

import _nstep_reference as N

pytestmark = pytest.mark.gpu

OBS_FLOATS = (1, 3, 7, 8, 9, 11, 12, 15, 16, 17, 81)
MASK_BYTES = (0, 1, 3, 4, 5, 7, 8, 9, 45)
GUARD_F, GUARD_B = 7.0, 9


def _lib():
    import generalsreinforcementlearning_amd as g
    return g.load()


def _check(rc, what):
    from generalsreinforcementlearning_amd._lib import check
    check(rc, what)


def _at_offset(rows, off, guard):
    """rows as one device allocation of 3 + rows.size + 3 elements with rows starting `off` elements in; -> (flat, view of rows)"""
    import torch
    flat = torch.full((rows.size + 6,), guard, dtype=torch.from_numpy(rows[:0]).dtype, device="cuda")
    flat[off:off + rows.size] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).cuda()
    return flat, flat[off:off + rows.size]


def _guarded(flat, off, size, guard):
    """the payload of a guarded flat output, after checking that nothing outside it was written"""
    got = flat.cpu().numpy()
    assert (got[:off] == guard).all() and (got[off + size:] == guard).all(), "a store outside the rows"
    return got[off:off + size]


# ---- row movers ----------------------------------------------------------------------------------------------------------
def _traj_gather(L, rng, M, F, K):
    """gvec_traj_gather of M rows at all 16 (source, destination) offsets, floats and mask bytes alike"""
    import torch
    from generalsreinforcementlearning_amd._lib import TrajGatherArgs
    T, Nn = 2, 3
    obs = rng.standard_normal((T * Nn, F)).astype(np.float32)
    mask = rng.integers(0, 256, (T * Nn, K)).astype(np.uint8)
    pos = rng.integers(0, T * Nn, M)
    z = lambda dt: torch.zeros(T * Nn, dtype=dt, device="cuda")
    action, flags = z(torch.int64), torch.ones(T * Nn, dtype=torch.uint8, device="cuda")
    logp, value, ret, adv = z(torch.float32), z(torch.float32), z(torch.float32), z(torch.float32)
    d_pos = torch.from_numpy(pos).cuda()
    e = lambda dt: torch.zeros(M, dtype=dt, device="cuda")
    o = dict(action=e(torch.int64), logp=e(torch.float32), value=e(torch.float32), ret=e(torch.float32), adv=e(torch.float32), weight=e(torch.float32))
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    for so in range(4):
        _, s_obs = _at_offset(obs, so, GUARD_F)
        _, s_mask = _at_offset(mask, so, GUARD_B)
        for do in range(4):
            o_obs = torch.full((M * F + 6,), GUARD_F, dtype=torch.float32, device="cuda")
            o_mask = torch.full((M * K + 6,), GUARD_B, dtype=torch.uint8, device="cuda")
            a = TrajGatherArgs(T=T, N=Nn, M=M, obs_floats=F, mask_bytes=K, pos=d_pos.data_ptr(), obs=s_obs.data_ptr(),
                               mask=s_mask.data_ptr() if K else None, action=action.data_ptr(), logp=logp.data_ptr(), value=value.data_ptr(),
                               ret=ret.data_ptr(), adv=adv.data_ptr(), flags=flags.data_ptr(), stats=None,
                               out_obs=o_obs[do:].data_ptr(), out_mask=o_mask[do:].data_ptr() if K else None,
                               out_action=o["action"].data_ptr(), out_logp=o["logp"].data_ptr(), out_value=o["value"].data_ptr(),
                               out_ret=o["ret"].data_ptr(), out_adv=o["adv"].data_ptr(), out_weight=o["weight"].data_ptr(),
                               rejected=rejected.data_ptr())
            _check(L.gvec_traj_gather(0, torch.cuda.current_stream().cuda_stream, C.byref(a)), "gvec_traj_gather")
            torch.cuda.synchronize()
            got = _guarded(o_obs, do, M * F, GUARD_F).reshape(M, F)
            assert got.view(np.uint32).tobytes() == obs[pos].view(np.uint32).tobytes(), (F, so, do)
            assert np.array_equal(_guarded(o_mask, do, M * K, GUARD_B).reshape(M, K), mask[pos]), (K, so, do)
    assert int(rejected.item()) == 0 and (o["weight"].cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("i", range(len(OBS_FLOATS)), ids=[f"f{f}" for f in OBS_FLOATS])
def test_traj_gather_rows_at_every_alignment(i):
    """M = 5: eight wavefronts per row (shift 3)"""
    _traj_gather(_lib(), np.random.default_rng(i), 5, OBS_FLOATS[i], MASK_BYTES[i % len(MASK_BYTES)])


def test_traj_gather_one_wavefront_per_row():
    """M = 16,384 rows of 17 floats: shift 0"""
    _traj_gather(_lib(), np.random.default_rng(99), 16384, 17, 5)


@pytest.mark.parametrize("M", [5000, 10000])
def test_traj_gather_two_and_four_wavefronts_per_row(M):
    """M = 10,000: shift 1; M = 5,000: shift 2 (split_shift: the smallest shift with M << shift >= 16,384)"""
    _traj_gather(_lib(), np.random.default_rng(M), M, 17, 5)


def _nstep_gather(L, rng, k, F):
    """gvec_nstep_gather with n_step 1 (no links: ring[idx] row for row) at all 16 (ring, output) offsets"""
    import torch
    from generalsreinforcementlearning_amd._lib import NstepGatherArgs
    cap = 6
    state, nxt = (rng.standard_normal((cap, F)).astype(np.float32) for _ in range(2))
    idx = rng.integers(0, cap, k)
    d_idx = torch.from_numpy(idx).cuda()
    action, reward = torch.arange(cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.float64, device="cuda")
    done = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    counters = torch.tensor([0, cap, cap, 0], dtype=torch.int64, device="cuda")
    o = dict(action=torch.zeros(k, dtype=torch.int64, device="cuda"), ret=torch.zeros(k, dtype=torch.float64, device="cuda"),
             discount=torch.zeros(k, dtype=torch.float64, device="cuda"), done=torch.zeros(k, dtype=torch.uint8, device="cuda"),
             steps=torch.zeros(k, dtype=torch.int32, device="cuda"), last_idx=torch.zeros(k, dtype=torch.int64, device="cuda"))
    for so in range(4):
        _, s0 = _at_offset(state, so, GUARD_F)
        _, s1 = _at_offset(nxt, (so + 1) & 3, GUARD_F)          # the two rows of a sample need not be aligned alike either
        for do in range(4):
            o0 = torch.full((k * F + 6,), GUARD_F, dtype=torch.float32, device="cuda")
            o1 = torch.full((k * F + 6,), GUARD_F, dtype=torch.float32, device="cuda")
            a = NstepGatherArgs()
            a.k, a.capacity, a.n_step, a.obs_floats, a.gamma = k, cap, 1, F, 0.99
            for name, tensor in (("idx", d_idx), ("ring_state", s0), ("ring_next_state", s1), ("ring_action", action), ("ring_reward", reward),
                                 ("ring_done", done), ("ring_counters", counters), ("state", o0[do:]), ("next_state", o1[(do + 2) & 3:])) + tuple(o.items()):
                setattr(a, name, tensor.data_ptr())
            a.ring_succ = None
            _check(L.gvec_nstep_gather(0, None, C.byref(a)), "gvec_nstep_gather")
            torch.cuda.synchronize()
            got0 = _guarded(o0, do, k * F, GUARD_F).reshape(k, F)
            got1 = _guarded(o1, (do + 2) & 3, k * F, GUARD_F).reshape(k, F)
            assert got0.view(np.uint32).tobytes() == state[idx].view(np.uint32).tobytes(), (F, so, do)
            assert got1.view(np.uint32).tobytes() == nxt[idx].view(np.uint32).tobytes(), (F, so, do)
    assert np.array_equal(o["action"].cpu().numpy(), idx) and np.array_equal(o["last_idx"].cpu().numpy(), idx)


@pytest.mark.parametrize("F", OBS_FLOATS)
def test_nstep_gather_rows_at_every_alignment(F):
    _nstep_gather(_lib(), np.random.default_rng(F), 5, F)


def test_nstep_gather_one_wavefront_per_row():
    _nstep_gather(_lib(), np.random.default_rng(98), 16384, 17)


@pytest.mark.parametrize("k", [5000, 10000])
def test_nstep_gather_two_and_four_wavefronts_per_row(k):
    """k = 10,000: shift 1; k = 5,000: shift 2"""
    _nstep_gather(_lib(), np.random.default_rng(k), k, 17)


# ---- the one-workgroup scan ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 1023, 1025, 2049])
def test_packed_stream_offsets_are_the_cumsum_of_the_counts(B):
    import generalsreinforcementlearning_amd as g
    eng = g.VecEngine(B, 4, 4, 2)
    eng.reset_generated(3)
    try:
        for turn in range(3):
            eng.step(eng.agent_actions(7 + turn))
            for full in (False, True):
                kind, count, upd = eng.stream_deltas(0)
                count = np.where(full & (kind == 2), 16, count).astype(np.int64) if full else count.astype(np.int64)
                pk, off, pupd = eng.stream_deltas_packed(0, full_tiles=full)
                assert np.array_equal(pk, kind)
                assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(count)), (B, turn, full)
                assert len(pupd) == int(count.sum())
                if not full:
                    assert np.array_equal(pupd, np.concatenate([upd[e, : count[e]] for e in range(B)]))
        assert count.sum() > 0
    finally:
        eng.close()


@pytest.mark.parametrize("total,groups", [(1000, 1), (1025, 2), (1024 * 1024, 1024), (1024 * 1024 + 1, 1025)])
def test_compact_at_the_scan_s_group_counts(total, groups):
    """gvec_traj_compact counts the valid rows per 1,024 positions and scans the counts"""
    import torch
    from generalsreinforcementlearning_amd._lib import TrajCompactArgs
    L = _lib()
    assert (total + 1023) // 1024 == groups
    flags = (np.random.default_rng(groups).random(total) < 0.3).astype(np.uint8)        # bit 0: GVEC_TRAJ_VALID
    d_flags = torch.from_numpy(flags).cuda()
    idx = torch.full((total + 2,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(1, total)), dtype=torch.uint8, device="cuda")
    a = TrajCompactArgs(T=1, N=total, flags=d_flags.data_ptr(), idx=idx[1:].data_ptr(), count=count[1:].data_ptr(), scratch=scratch.data_ptr())
    _check(L.gvec_traj_compact(0, torch.cuda.current_stream().cuda_stream, C.byref(a)), "gvec_traj_compact")
    torch.cuda.synchronize()
    want = np.flatnonzero(flags)
    assert count.tolist() == [-1, want.size, -1]
    got = idx.cpu().numpy()
    assert got[0] == -7 and np.array_equal(got[1:1 + want.size], want) and (got[1 + want.size:] == -7).all()


@pytest.mark.parametrize("workers,groups", [(64, 1), (65, 2), (5000, 79), (10000, 157), (65536, 1024), (65537, 1025)])   # 5,000 / 10,000: the copy's shift 2 / 1
def test_pool_collect_at_the_scan_s_group_counts(workers, groups):
    """One gvec_pool_collect step with obs_floats = 1 from a ring that is about to wrap: the ring against RingModel (the host
    restatement of tests/test_nstep_replay.py), the result rows against the over-workers in ascending order."""
    import torch
    from generalsreinforcementlearning_amd._lib import CollectArgs
    L = _lib()
    assert (workers + 63) // 64 == groups
    rng = np.random.default_rng(workers)
    cap, limit, start = workers + 50, 4, workers + 45                      # the cursor five slots before the ring's end
    x = dict(state=rng.standard_normal((workers, 1)).astype(np.float32), next_state=rng.standard_normal((workers, 1)).astype(np.float32),
             action=rng.integers(0, 1000, workers).astype(np.int64), reward=rng.standard_normal(workers),
             terminated=(rng.random(workers) < 0.2).astype(np.uint8), truncated=(rng.random(workers) < 0.1).astype(np.uint8),
             was_reset=(rng.random(workers) < 0.3).astype(np.uint8))
    ep_reward, ep_length = rng.standard_normal(workers), rng.integers(0, limit, workers).astype(np.int64)
    m = N.RingModel(workers, cap, limit, 1)
    m.cursor, m.size, m.total, m.length = start, start, start, ep_length.copy()
    live = ~x["was_reset"].astype(bool)
    over = live & ((x["terminated"] | x["truncated"]).astype(bool) | (ep_length + 1 >= limit))
    m.step(x)
    dev = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    z = lambda n, dt, fill=0: torch.full((n,), fill, dtype=dt, device="cuda")
    ring = dict(ring_state=z(cap + 2, torch.float32, GUARD_F), ring_next_state=z(cap + 2, torch.float32, GUARD_F), ring_action=z(cap, torch.int64),
                ring_reward=z(cap, torch.float64), ring_done=z(cap, torch.uint8))
    res = dict(result_reward=z(workers + 2, torch.float64, GUARD_F), result_length=z(workers + 2, torch.int32, GUARD_B),
               result_worker=z(workers + 2, torch.int32, GUARD_B))
    counters = torch.tensor([start, start, start, 0], dtype=torch.int64, device="cuda")
    pool_counters = z(4, torch.int64)
    d_ep_reward, d_ep_length = torch.from_numpy(ep_reward).cuda(), torch.from_numpy(ep_length).cuda()
    needs_reset = z(workers, torch.uint8)
    scratch = z((int(L.gvec_pool_collect_scratch_bytes(workers)) + 7) // 8, torch.int64)
    a = CollectArgs()
    a.num_envs, a.obs_floats, a.max_steps_per_episode, a.capacity, a.result_capacity = workers, 1, limit, cap, workers
    for name, tensor in tuple(dev.items()) + (("ring_counters", counters), ("episode_reward", d_ep_reward), ("episode_length", d_ep_length),
                                              ("pool_counters", pool_counters), ("scratch", scratch), ("needs_reset", needs_reset)):
        setattr(a, name, tensor.data_ptr())
    for name, tensor in tuple(ring.items()) + tuple(res.items()):
        guarded = name in ("ring_state", "ring_next_state") or name in res
        setattr(a, name, (tensor[1:] if guarded else tensor).data_ptr())
    assert L.gvec_pool_collect(0, None, C.byref(a)) == 0, L.gvec_last_error()
    torch.cuda.synchronize()
    assert counters.tolist() == [m.cursor, m.size, m.total, 0] and m.cursor < start          # it wrapped
    new = (start + np.arange(int(live.sum()))) % cap                                           # the slots of this step, in worker order
    assert np.array_equal(m.worker[new], np.flatnonzero(live))
    for f, want in (("ring_state", m.state[:, 0]), ("ring_next_state", m.next_state[:, 0])):
        got = _guarded(ring[f], 1, cap, GUARD_F)
        assert got[new].view(np.uint32).tobytes() == want[new].view(np.uint32).tobytes(), f
        untouched = np.setdiff1d(np.arange(cap), new)
        assert (got[untouched] == GUARD_F).all(), f
    assert np.array_equal(ring["ring_action"].cpu().numpy()[new], m.action[new])
    assert np.array_equal(ring["ring_reward"].cpu().numpy()[new], m.reward[new])
    assert np.array_equal(ring["ring_done"].cpu().numpy()[new].astype(bool), m.done[new])
    ended = np.flatnonzero(over)
    assert pool_counters.tolist()[:3] == [ended.size, ended.size, 0] and ended.size > 0
    got_worker = _guarded(res["result_worker"], 1, workers, GUARD_B)
    assert np.array_equal(got_worker[:ended.size], ended) and (got_worker[ended.size:] == GUARD_B).all()
    assert np.array_equal(_guarded(res["result_length"], 1, workers, GUARD_B)[:ended.size], ep_length[ended] + 1)
    assert np.array_equal(_guarded(res["result_reward"], 1, workers, GUARD_F)[:ended.size], ep_reward[ended] + x["reward"][ended])
