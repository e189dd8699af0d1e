"""The on-policy rollout path on the GPU: zero-copy observation slots of GeneralsSelfPlayVecEnv.step, the gvec_traj_* kernels
against their numpy restatement (tests/_gae_reference.py), and SelfPlayRolloutBuffer end to end."""
import ctypes as C

import numpy as np
import pytest

import _gae_reference as R

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _lib():
    import generalsreinforcementlearning_amd as g
    return g.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    from generalsreinforcementlearning_amd._lib import check
    check(rc, what)


def _actions_from_mask(mask, gen):
    """One valid action per learner, drawn from its mask (action 0 for a learner that has none)."""
    import torch
    B, L, K = mask.shape
    m = mask.reshape(B * L, K).float()
    m[:, 0] += (m.sum(1) == 0).float()
    return torch.multinomial(m, 1, generator=gen).reshape(B, L)


# ---- 1. zero-copy observation slots --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,P,B", [(15, 15, 2, 5), (20, 20, 4, 3)], ids=["15x15_p2", "20x20_p4"])
def test_step_into_slots_is_bit_equal(w, h, P, B):
    import torch
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    T = 40
    mk = lambda: GeneralsSelfPlayVecEnv(B, w, h, P, max_turns=15, seed=11, board_pool=16, device_outputs=True)
    plain, slotted = mk(), mk()
    n_obs, n_mask = B * P * 9 * w * h, B * P * 5 * w * h
    # the stores start 12 bytes / 1 byte into their allocations: no slot is aligned to more than its dtype
    obs_flat = torch.zeros((T + 1) * n_obs + 3, dtype=torch.float32, device="cuda")
    mask_flat = torch.zeros((T + 1) * n_mask + 1, dtype=torch.uint8, device="cuda")
    obs_store, mask_store = obs_flat[3:].view(T + 1, n_obs), mask_flat[1:].view(T + 1, n_mask)
    assert (n_mask % 256) != 0 and all(obs_store[k].data_ptr() % 256 for k in range(T + 1))
    assert any(obs_store[k].data_ptr() % 16 for k in range(T + 1)) and any(mask_store[k].data_ptr() % 4 for k in range(T + 1))
    (o0, i0), (o1, i1) = plain.reset(), slotted.reset()
    assert torch.equal(o0, o1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    mask = i0["valid_actions_mask"]
    resets = 0
    for k in range(T):
        a = _actions_from_mask(mask, gen)
        ob0, r0, te0, tr0, in0 = plain.step(a)
        ob1, r1, te1, tr1, in1 = slotted.step(a.clone(), obs_out=obs_store[k + 1], mask_out=mask_store[k + 1])
        assert ob1.data_ptr() == obs_store[k + 1].data_ptr() and in1["valid_actions_mask"].data_ptr() == mask_store[k + 1].data_ptr()
        assert ob1.shape == ob0.shape and in1["valid_actions_mask"].shape == in0["valid_actions_mask"].shape
        assert torch.equal(ob0.view(torch.int32), ob1.view(torch.int32)), k
        assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(te0, te1) and torch.equal(tr0, tr1), k
        for key in in0:
            assert torch.equal(in0[key], in1[key]), (k, key)
        resets += int(in0["reset"].sum())
        mask = in0["valid_actions_mask"]
    assert resets >= B                       # max_turns < T: every env was re-dealt on the way
    # the slots a later step did not write still hold what their own step wrote
    assert torch.equal(obs_store[T].view(B, P, 9, h, w), ob0)
    assert float(obs_flat[:3].abs().sum()) == 0.0 and int(mask_flat[0]) == 0
    with pytest.raises(ValueError):
        slotted.step(a, obs_out=obs_store[1])
    with pytest.raises(ValueError):
        slotted.step(a, obs_out=obs_store[1].double(), mask_out=mask_store[1])
    with pytest.raises(ValueError):
        slotted.step(a, obs_out=obs_store[1][:-1], mask_out=mask_store[1])
    with pytest.raises(ValueError):
        slotted.step(a, obs_out=obs_store[1].cpu(), mask_out=mask_store[1])
    plain.close()
    slotted.close()


# ---- 2. gvec_traj_record -------------------------------------------------------------------------------------------------
def test_record_against_the_restatement():
    import torch
    from generalsreinforcementlearning_amd._lib import TrajRecordArgs
    B, Lr, T = 37, 3, 6
    N = B * Lr
    rng = np.random.default_rng(0)
    # step 0: every combination of (reset, terminated, truncated) x (alive, alive_state) appears; env 0's learner 1 dies at
    # step 1, env 0 is re-dealt at step 2 (everyone alive again at step 3), stream N-1 is dead for the whole rollout
    alive_state = np.ones(N, np.uint8)
    alive_state[N - 1] = 0
    d_state = _dev(alive_state)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    action, logp, value = z((T, N), torch.int64), z((T, N), torch.float32), z((T + 1, N), torch.float32)
    reward, flags = z((T, N), torch.float64), torch.full((T, N), 0xEE, dtype=torch.uint8, device="cuda")
    want_flags = np.zeros((T, N), np.uint8)
    steps = []
    seen = set()
    for t in range(T):
        rs, te, tr = (rng.integers(0, 2, B).astype(np.uint8) for _ in range(3))
        al = rng.integers(0, 2, N).astype(np.uint8)
        if t == 0:
            for b in range(8):
                rs[b], te[b], tr[b] = b & 1, (b >> 1) & 1, (b >> 2) & 1
            rs[0], al[0], al[1] = 0, 1, 1
        if t == 1:
            rs[0] = te[0] = tr[0] = 0
            al[0], al[1] = 1, 0
        if t == 2:
            rs[0], al[0], al[1] = 1, 1, 1
        if t == 3:
            rs[0] = 0
        al[N - 1] = 0
        st = dict(a=rng.integers(0, 1125, N), lp=rng.standard_normal(N).astype(np.float32), v=rng.standard_normal(N).astype(np.float32),
                  r=rng.standard_normal(N), rs=rs, te=te, tr=tr, al=al)
        want_flags[t], new_state = R.record_flags(rs, te, tr, al, alive_state, Lr)
        for n in range(N):
            seen.add((rs[n // Lr], te[n // Lr], tr[n // Lr], al[n], alive_state[n]))
        alive_state = new_state
        keep = [_dev(st[k]) for k in ("a", "lp", "v", "r", "rs", "te", "tr", "al")]
        a = TrajRecordArgs(T=T, t=t, num_envs=B, num_learners=Lr, step_action=keep[0].data_ptr(), step_logp=keep[1].data_ptr(),
                           step_value=keep[2].data_ptr(), step_reward=keep[3].data_ptr(), reset=keep[4].data_ptr(),
                           terminated=keep[5].data_ptr(), truncated=keep[6].data_ptr(), alive=keep[7].data_ptr(),
                           alive_state=d_state.data_ptr(), action=action.data_ptr(), logp=logp.data_ptr(), value=value.data_ptr(),
                           reward=reward.data_ptr(), flags=flags.data_ptr())
        _check(_lib().gvec_traj_record(0, _stream(), C.byref(a)), "gvec_traj_record")
        steps.append((st, keep))
    torch.cuda.synchronize()
    assert len(seen) == 32                                    # every combination of the five inputs
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    assert np.array_equal(d_state.cpu().numpy(), alive_state)
    assert want_flags[1, 1] == 7 and want_flags[2, 1] == 0 and want_flags[3, 1] & 1 and not want_flags[:, N - 1].any()
    for t, (st, _) in enumerate(steps):
        assert np.array_equal(action[t].cpu().numpy(), st["a"]) and np.array_equal(logp[t].cpu().numpy(), st["lp"])
        assert np.array_equal(value[t].cpu().numpy(), st["v"]) and np.array_equal(reward[t].cpu().numpy(), st["r"])
    assert not value[T].cpu().numpy().any()


# ---- 3. gvec_traj_gae ----------------------------------------------------------------------------------------------------
def _run_gae(reward, value, flags, gamma, lam):
    import torch
    from generalsreinforcementlearning_amd._lib import TrajGaeArgs
    T, N = reward.shape
    L = _lib()
    d = [_dev(reward), _dev(value), _dev(flags)]
    adv, ret = (torch.full((T, N), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    stats = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(T, N)), dtype=torch.uint8, device="cuda")
    a = TrajGaeArgs(T=T, N=N, gamma=gamma, lam=lam, reward=d[0].data_ptr(), value=d[1].data_ptr(), flags=d[2].data_ptr(),
                    adv=adv.data_ptr(), ret=ret.data_ptr(), stats=stats.data_ptr(), scratch=scratch.data_ptr())
    _check(L.gvec_traj_gae(0, _stream(), C.byref(a)), "gvec_traj_gae")
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy(), stats.cpu().numpy()


def _assert_gae(reward, value, flags, gamma, lam, ctx):
    T, N = reward.shape
    adv, ret, st = _run_gae(reward, value, flags, gamma, lam)
    want_adv, want_ret = R.gae(reward, value, flags, gamma, lam)
    da, dr = R.ulp_diff(adv, want_adv.astype(np.float32)), R.ulp_diff(ret, want_ret.astype(np.float32))
    print(f"{ctx}: max ulp adv {da.max()} ret {dr.max()}")
    assert da.max() <= 1 and dr.max() <= 1, ctx
    want = R.stats(adv, flags)
    s_abs, s_sq = R.stats_abs(adv, flags)
    print(f"{ctx}: stats {st} want {want}")
    assert st[0] == want[0] and st[3] == 0.0, ctx
    assert abs(st[1] - want[1]) <= T * N * 2.0 ** -53 * s_abs and abs(st[2] - want[2]) <= T * N * 2.0 ** -53 * s_sq, ctx
    adv2, ret2, st2 = _run_gae(reward, value, flags, gamma, lam)
    assert adv.tobytes() == adv2.tobytes() and ret.tobytes() == ret2.tobytes() and st.tobytes() == st2.tobytes(), ctx
    return adv, ret, st


# T = 33 and 95: a full 32-row chunk, then a partial one; N = 16,448: 257 per-wavefront partials, so a thread of the
# statistics' second stage (stride 256) adds two
GAE_CASES = [(T, N) for T in (1, 2, 33, 95, 128, 512) for N in (1, 63, 64, 65, 8192)] + [(2, 16448)]


@pytest.mark.parametrize("T,N", GAE_CASES, ids=[f"{N}-{T}" for T, N in GAE_CASES])
def test_gae_against_the_restatement(T, N):
    rng = np.random.default_rng(1000 * T + N)
    reward, value, flags = R.random_rollout(rng, T, N)
    _assert_gae(reward, value, flags, 0.99, 0.95, f"T{T} N{N}")


@pytest.mark.parametrize("pattern", ["cut_everywhere", "no_cut", "all_invalid", "terminal_everywhere"])
def test_gae_flag_extremes(pattern):
    rng = np.random.default_rng(3)
    T, N = 128, 65
    reward, value, _ = R.random_rollout(rng, T, N)
    f = {"cut_everywhere": R.VALID | R.CUT, "no_cut": R.VALID, "all_invalid": 0, "terminal_everywhere": R.VALID | R.CUT | R.TERMINAL}[pattern]
    flags = np.full((T, N), f, np.uint8)
    adv, ret, st = _assert_gae(reward, value, flags, 0.99, 0.95, pattern)
    if pattern == "all_invalid":
        assert not adv.any() and np.array_equal(ret, value[:-1]) and not st.any()


# ---- 4. gvec_traj_compact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,p_invalid", [(1, 1, 0.0), (1, 1, 1.0), (7, 63, 0.3), (128, 65, 0.05), (33, 1024, 0.5), (64, 8192, 0.02), (5, 1023, 1.0)])
def test_compact_equals_flatnonzero(T, N, p_invalid):
    import torch
    from generalsreinforcementlearning_amd._lib import TrajCompactArgs
    L = _lib()
    rng = np.random.default_rng(T * 31 + N)
    _, _, flags = R.random_rollout(rng, T, N, p_invalid=p_invalid)
    d_flags = _dev(flags)
    idx = torch.full((T * N,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(T, N)), dtype=torch.uint8, device="cuda")
    a = TrajCompactArgs(T=T, N=N, flags=d_flags.data_ptr(), idx=idx.data_ptr(), count=count.data_ptr(), scratch=scratch.data_ptr())
    _check(L.gvec_traj_compact(0, _stream(), C.byref(a)), "gvec_traj_compact")
    torch.cuda.synchronize()
    want = R.compact(flags)
    assert int(count.item()) == want.size
    got = idx.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == -7)


# ---- 5. gvec_traj_gather -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,M", [(15, 1), (15, 777), (20, 130), (15, 20000), (3, 65), (1, 65)],
                         ids=["15x15_m1", "15x15_m777", "20x20_m130", "15x15_m20000", "3x3_m65", "1x1_m65"])
@pytest.mark.parametrize("normalise", [False, True])
def test_gather_against_fancy_indexing(w, M, normalise):
    import torch
    from generalsreinforcementlearning_amd._lib import TrajGatherArgs
    L = _lib()
    T, N = 5, 13
    F, K = 9 * w * w, 5 * w * w
    rng = np.random.default_rng(w * 1000 + M)
    obs = rng.standard_normal((T + 1, N, F)).astype(np.float32)
    mask = rng.integers(0, 2, (T + 1, N, K)).astype(np.uint8)
    reward, value, flags = R.random_rollout(rng, T, N, p_invalid=0.2)
    action, logp = rng.integers(0, K, (T, N)), rng.standard_normal((T, N)).astype(np.float32)
    adv, ret = (x.astype(np.float32) for x in R.gae(reward, value, flags, 0.99, 0.95))
    st = R.stats(adv, flags)
    pos = rng.integers(0, T * N, M)                       # with replacement: repeated positions
    if M >= 65:
        pos[[3, 17, 40, 64]] = [-1, T * N, 2 ** 40, -2 ** 62]
        pos[5] = pos[6] = T * N - 1
        pos[7] = 0
    want = R.gather(pos, obs, mask, action, logp, value, ret, adv, flags, st if normalise else None)
    d = {k: _dev(v) for k, v in dict(pos=pos, obs=obs, mask=mask, action=action, logp=logp, value=value, ret=ret, adv=adv, flags=flags, stats=st).items()}
    # outputs start 4 bytes (the masks: 1 byte) into their allocations, so output rows are misaligned in their own way
    o_obs = torch.full((M * F + 1,), 7.0, dtype=torch.float32, device="cuda")
    o_mask = torch.full((M * K + 1,), 9, dtype=torch.uint8, device="cuda")
    e = lambda dt: torch.full((M,), 5, dtype=dt, device="cuda")
    o = dict(action=e(torch.int64), logp=e(torch.float32), value=e(torch.float32), ret=e(torch.float32), adv=e(torch.float32), weight=e(torch.float32))
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = TrajGatherArgs(T=T, N=N, M=M, obs_floats=F, mask_bytes=K, pos=d["pos"].data_ptr(), obs=d["obs"].data_ptr(), mask=d["mask"].data_ptr(),
                       action=d["action"].data_ptr(), logp=d["logp"].data_ptr(), value=d["value"].data_ptr(), ret=d["ret"].data_ptr(),
                       adv=d["adv"].data_ptr(), flags=d["flags"].data_ptr(), stats=d["stats"].data_ptr() if normalise else None,
                       out_obs=o_obs[1:].data_ptr(), out_mask=o_mask[1:].data_ptr(), out_action=o["action"].data_ptr(),
                       out_logp=o["logp"].data_ptr(), out_value=o["value"].data_ptr(), out_ret=o["ret"].data_ptr(),
                       out_adv=o["adv"].data_ptr(), out_weight=o["weight"].data_ptr(), rejected=rejected.data_ptr())
    _check(L.gvec_traj_gather(0, _stream(), C.byref(a)), "gvec_traj_gather")
    torch.cuda.synchronize()
    got_obs, got_mask = o_obs.cpu().numpy(), o_mask.cpu().numpy()
    assert got_obs[0] == 7.0 and got_mask[0] == 9                 # nothing written in front of the first row
    assert got_obs[1:].reshape(M, F).view(np.uint32).tobytes() == want["obs"].view(np.uint32).tobytes()
    assert np.array_equal(got_mask[1:].reshape(M, K), want["mask"])
    for k in ("action", "logp", "value", "ret", "weight"):
        assert np.array_equal(o[k].cpu().numpy(), want[k]), k
    got_adv = o["adv"].cpu().numpy()
    if normalise:
        ulp = R.ulp_diff(got_adv, want["adv"].astype(np.float32))
        print(f"normalised adv: max ulp {ulp.max()}")
        assert ulp.max() <= 2
    else:
        assert np.array_equal(got_adv, want["adv"])
    assert int(rejected.item()) == want["rejected"] and want["rejected"] == (4 if M >= 65 else 0)


# ---- 6 - 8. SelfPlayRolloutBuffer ----------------------------------------------------------------------------------------
def _collect(buf, gen, rng_value):
    """One full rollout with actions drawn from the mask; returns the per-step host copies of what the env returned."""
    import torch
    log = []
    B, L = buf.num_envs, buf.num_learners
    while not buf.full:
        a = _actions_from_mask(buf.valid_actions_mask, gen)
        logp = torch.randn(B, L, device="cuda", generator=gen)
        value = torch.randn(B, L, device="cuda", generator=gen)
        _, r, te, tr, info = buf.step(a, logp, value)
        log.append(dict(a=a.cpu().numpy(), logp=logp.cpu().numpy(), value=value.cpu().numpy(), r=r.cpu().numpy(), te=te.cpu().numpy(),
                        tr=tr.cpu().numpy(), rs=info["reset"].cpu().numpy(), al=info["alive"].cpu().numpy()))
    return log


def _host_flags(log, alive_state, L):
    flags = []
    for s in log:
        f, alive_state = R.record_flags(s["rs"], s["te"], s["tr"], s["al"].reshape(-1), alive_state, L)
        flags.append(f)
    return np.stack(flags), alive_state


def test_buffer_end_to_end():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, L, T = 24, 2, 64
    N = B * L
    env = GeneralsSelfPlayVecEnv(B, 8, 8, 2, max_turns=20, seed=3, board_pool=16, device_outputs=True)
    buf = g.SelfPlayRolloutBuffer(env, T, gamma=0.99, gae_lambda=0.95)
    buf.begin(*env.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    with pytest.raises(RuntimeError):
        buf.finish(torch.zeros(B, L, device="cuda"))
    log = _collect(buf, gen, None)
    assert buf.full
    with pytest.raises(RuntimeError):
        buf.step(torch.zeros(B, L, dtype=torch.int64, device="cuda"), torch.zeros(B, L, device="cuda"), torch.zeros(B, L, device="cuda"))
    last_value = torch.randn(B, L, device="cuda", generator=gen)
    buf.finish(last_value)
    torch.cuda.synchronize()
    flags, alive_state = _host_flags(log, np.ones(N, np.uint8), L)
    assert np.array_equal(buf.flags.cpu().numpy(), flags)
    assert np.array_equal(buf.alive_state.cpu().numpy(), alive_state)
    trunc, resets = np.stack([s["tr"] for s in log]), np.stack([s["rs"] for s in log])
    assert trunc.any(0).all() and resets.any(0).all()           # every env: at least one truncation and one re-deal row
    assert np.array_equal(resets[1:], (trunc | np.stack([s["te"] for s in log]))[:-1])
    reward = np.stack([s["r"].reshape(-1) for s in log])
    value = np.concatenate([np.stack([s["value"].reshape(-1) for s in log]), last_value.cpu().numpy().reshape(1, -1)]).astype(np.float32)
    assert np.array_equal(buf.reward.cpu().numpy(), reward) and np.array_equal(buf.value.cpu().numpy(), value)
    assert np.array_equal(buf.action.cpu().numpy(), np.stack([s["a"].reshape(-1) for s in log]))
    want_adv, want_ret = R.gae(reward, value, flags, 0.99, 0.95)
    adv, ret = buf.advantages.cpu().numpy(), buf.returns.cpu().numpy()
    assert adv.shape == (T, B, L) and buf.valid.shape == (T, B, L)
    da = R.ulp_diff(adv.reshape(T, N), want_adv.astype(np.float32))
    dr = R.ulp_diff(ret.reshape(T, N), want_ret.astype(np.float32))
    print(f"end to end: max ulp adv {da.max()} ret {dr.max()}; valid rows {int((flags & 1).sum())} of {T * N}")
    assert da.max() <= 1 and dr.max() <= 1
    assert np.array_equal(buf.valid.cpu().numpy().reshape(T, N), (flags & 1) != 0)
    st, want_st = buf.stats.cpu().numpy(), R.stats(adv.reshape(T, N), flags)
    s_abs, s_sq = R.stats_abs(adv.reshape(T, N), flags)
    assert st[0] == want_st[0] and abs(st[1] - want_st[1]) <= T * N * 2.0 ** -53 * s_abs and abs(st[2] - want_st[2]) <= T * N * 2.0 ** -53 * s_sq

    # minibatches: every position exactly once per epoch; the rows are the stores' rows
    obs_np, mask_np = buf.obs_store.cpu().numpy().reshape(T + 1, N, -1), buf.mask_store.cpu().numpy().reshape(T + 1, N, -1)
    for compact in (False, True):
        seen = []
        for batch in buf.minibatches(1000, epochs=1, normalize=False, compact=compact, seed=4):
            p = batch["index"].cpu().numpy()
            seen.append(p)
            assert np.array_equal(batch["obs"].cpu().numpy().reshape(p.size, -1), obs_np.reshape((T + 1) * N, -1)[p])
            assert np.array_equal(batch["valid_actions_mask"].cpu().numpy(), mask_np.reshape((T + 1) * N, -1)[p].astype(bool))
            assert np.array_equal(batch["advantages"].cpu().numpy(), adv.reshape(-1)[p])
            assert np.array_equal(batch["weight"].cpu().numpy(), ((flags.reshape(-1)[p] & 1) != 0).astype(np.float32))
        seen = np.sort(np.concatenate(seen))
        assert np.array_equal(seen, R.compact(flags) if compact else np.arange(T * N))
    assert int(buf.rejected.item()) == 0

    env.close()


def test_next_rollout_carries_the_episode_over():
    """7. Slot T becomes slot 0, alive_state carries over, and row 0 of the next rollout is invalid for an env whose last
    step truncated (horizon == max_turns: the first rollout's last step is every running env's truncation)."""
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, L, T = 24, 2, 20
    env = GeneralsSelfPlayVecEnv(B, 8, 8, 2, max_turns=T, seed=3, board_pool=16, device_outputs=True)
    buf = g.SelfPlayRolloutBuffer(env, T)
    buf.begin(*env.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(10)
    log = _collect(buf, gen, None)
    buf.finish(torch.zeros(B, L, device="cuda"))
    _, alive_state = _host_flags(log, np.ones(B * L, np.uint8), L)
    slot_T, mask_T = buf.obs_store[T].clone(), buf.mask_store[T].clone()
    just_cut = (log[-1]["tr"] | log[-1]["te"]).astype(bool)
    assert log[-1]["tr"].any()
    buf.next_rollout()
    assert not buf.full and torch.equal(buf.obs, slot_T) and torch.equal(buf.obs_store[0], slot_T) and torch.equal(buf.mask_store[0], mask_T)
    assert np.array_equal(buf.alive_state.cpu().numpy(), alive_state)
    with pytest.raises(RuntimeError):
        buf.advantages
    log2 = _collect(buf, gen, None)
    buf.finish(torch.zeros(B, L, device="cuda"))
    torch.cuda.synchronize()
    flags2, _ = _host_flags(log2, alive_state, L)
    got2 = buf.flags.cpu().numpy()
    assert np.array_equal(got2, flags2)
    assert np.array_equal(log2[0]["rs"].astype(bool), just_cut)
    assert not got2[0].reshape(B, L)[just_cut].any() and got2[1].reshape(B, L)[just_cut].all()
    env.close()


def test_collection_does_not_synchronise():
    """buffer.step returns while the device still has earlier work queued (a stream query), and it can be captured into a
    graph - which a call that synchronised could not be."""
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, L, T = 64, 2, 8
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = GeneralsSelfPlayVecEnv(B, 15, 15, 2, max_turns=50, seed=1, board_pool=16, device_outputs=True)
        buf = g.SelfPlayRolloutBuffer(env, T)
        buf.begin(*env.reset())
        a = torch.zeros(B, L, dtype=torch.int64, device="cuda")
        lp, v = torch.zeros(B, L, device="cuda"), torch.ones(B, L, device="cuda")
        buf.step(a, lp, v)
        side.synchronize()
        x = torch.randn(8192, 8192, device="cuda")
        y = x
        for _ in range(40):                                     # some hundred milliseconds of queued work
            y = (x @ y) * 1e-2
        buf.step(a, lp, v)
        pending = not side.query()
        side.synchronize()
        assert pending, "buffer.step returned only after the queued work had finished"
        assert int(buf.flags[1].sum()) == B * L                 # the step did run afterwards

        sentinel = 0xEE
        buf.flags[2].fill_(sentinel)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            env.engine.set_stream(torch.cuda.current_stream().cuda_stream)
            buf.step(a, lp, v)
        env.engine.set_stream(side.cuda_stream)
        side.synchronize()
        assert int((buf.flags[2] == sentinel).sum()) == B * L   # captured, not run
        graph.replay()
        side.synchronize()
        assert int((buf.flags[2] == 1).sum()) == B * L and float(buf.obs_store[3].abs().sum()) > 0
        env.close()
