"""CPU-side checks of the rollout feature: the numpy restatement (tests/_gae_reference.py) against an independent
definition of GAE, its two closed-form limits, and the argument checks of the gvec_traj_* entry points, which answer before
any device is touched."""
import ctypes as C

import numpy as np
import pytest

import _gae_reference as R


def _deltas(reward, value, flags, gamma):
    v = value.astype(np.float64)
    term = (flags & R.TERMINAL) != 0
    return reward + gamma * np.where(term, 0.0, v[1:]) - v[:-1]


def _runs(flags, t, n):
    """The rows t, t+1, ... the advantage of row (t, n) sums over: up to the first CUT, or the last row before an invalid one."""
    T = flags.shape[0]
    k = t
    while True:
        yield k
        if (flags[k, n] & R.CUT) or k + 1 >= T or not (flags[k + 1, n] & R.VALID):
            return
        k += 1


@pytest.mark.parametrize("seed,T,N,gamma,lam", [(0, 40, 7, 0.99, 0.95), (1, 64, 5, 0.9, 0.5), (2, 17, 9, 1.0, 1.0), (3, 33, 4, 0.97, 0.0)])
def test_restatement_equals_the_direct_sum(seed, T, N, gamma, lam):
    rng = np.random.default_rng(seed)
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.1, p_invalid=0.1)
    adv, ret = R.gae(reward, value, flags, gamma, lam)
    delta = _deltas(reward, value, flags, gamma)
    want = np.zeros((T, N))
    scale = np.zeros((T, N))
    for t in range(T):
        for n in range(N):
            if flags[t, n] & R.VALID:
                terms = [(gamma * lam) ** (k - t) * delta[k, n] for k in _runs(flags, t, n)]
                want[t, n] = sum(terms)
                scale[t, n] = sum(abs(x) for x in terms)
    valid = (flags & R.VALID) != 0
    assert valid.any() and (~valid).any() and ((flags & R.CUT) != 0).any()
    assert np.all(np.abs(adv - want) <= T * 2.0 ** -52 * np.maximum(scale, 1e-300))
    assert np.all(adv[~valid] == 0.0) and np.all(ret[~valid] == value.astype(np.float64)[:-1][~valid])
    assert np.all(ret[valid] == (adv + value.astype(np.float64)[:-1])[valid])


def test_lambda_zero_is_the_td_error():
    rng = np.random.default_rng(5)
    reward, value, flags = R.random_rollout(rng, 50, 6, p_cut=0.1, p_invalid=0.1)
    adv, _ = R.gae(reward, value, flags, 0.99, 0.0)
    valid = (flags & R.VALID) != 0
    assert np.array_equal(adv[valid], _deltas(reward, value, flags, 0.99)[valid])


def test_lambda_one_is_the_discounted_return_plus_bootstrap():
    rng = np.random.default_rng(6)
    T, N, gamma = 48, 6, 0.97
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.1, p_invalid=0.1)
    _, ret = R.gae(reward, value, flags, gamma, 1.0)
    v = value.astype(np.float64)
    checked = 0
    for t in range(T):
        for n in range(N):
            if not (flags[t, n] & R.VALID):
                continue
            rows = list(_runs(flags, t, n))
            last = rows[-1]
            terms = [gamma ** (k - t) * reward[k, n] for k in rows]
            if not (flags[last, n] & R.TERMINAL):
                terms.append(gamma ** (last + 1 - t) * v[last + 1, n])        # the bootstrap at the cut
            # every value the telescoping sum passes through takes part in the rounding
            mag = sum(abs(x) for x in terms) + sum(2 * gamma ** (k - t) * abs(v[k, n]) for k in rows)
            np.testing.assert_allclose(ret[t, n], sum(terms), rtol=0, atol=T * 2.0 ** -52 * mag)
            checked += 1
    assert checked > T * N // 2


def test_record_flag_rule():
    # B = 4, L = 2: a re-dealt env, a terminated env, a truncated env, an env where learner 1 dies / was dead
    reset, term, trunc = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]
    alive, was = [1, 1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 1, 1]
    f, new = R.record_flags(reset, term, trunc, alive, was, 2)
    assert f.tolist() == [0, 0, 7, 7, 5, 5, 1, 7] and new.tolist() == alive
    f, _ = R.record_flags([0] * 4, [0] * 4, [0] * 4, alive, new, 2)
    assert f.tolist() == [1, 1, 1, 1, 1, 1, 1, 0]          # eliminated before the step: no transition


# ---- the ABI without a GPU ----
@pytest.fixture(scope="module")
def L():
    from generalsreinforcementlearning_amd.csrc import build as B
    B.build(verbose=False)
    import generalsreinforcementlearning_amd as g
    return g.load()


def _ptrs(cls, **kw):
    """An args struct whose every pointer is a (never dereferenced) non-NULL address."""
    a = cls()
    for name, typ in cls._fields_:
        if typ is C.c_void_p:
            setattr(a, name, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(L, fn, a):
    L.gvec_traj_record(0, None, None)          # leaves a known message behind
    before = L.gvec_last_error()
    rc = fn(0, None, C.byref(a) if a is not None else None)
    msg = L.gvec_last_error()
    assert rc == -1, rc                        # GVEC_E_INVALID
    assert msg and fn.__name__.encode() in msg, (before, msg)
    return msg


def test_traj_entry_points_refuse_bad_arguments_without_a_gpu(L):
    from generalsreinforcementlearning_amd._lib import TrajCompactArgs, TrajGaeArgs, TrajGatherArgs, TrajRecordArgs
    nan = float("nan")
    rec = dict(T=8, t=0, num_envs=4, num_learners=2)
    for bad in (dict(T=0), dict(num_envs=0), dict(num_learners=0), dict(t=-1), dict(t=8), dict(flags=None), dict(alive_state=None),
                dict(step_logp=None)):
        _refused(L, L.gvec_traj_record, _ptrs(TrajRecordArgs, **{**rec, **bad}))
    _refused(L, L.gvec_traj_record, None)
    gae = dict(T=8, N=4, gamma=0.99, lam=0.95)
    for bad in (dict(T=0), dict(N=0), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=nan), dict(lam=-0.1), dict(lam=1.01), dict(lam=nan),
                dict(stats=None), dict(scratch=None), dict(reward=None)):
        _refused(L, L.gvec_traj_gae, _ptrs(TrajGaeArgs, **{**gae, **bad}))
    _refused(L, L.gvec_traj_gae, None)
    for bad in (dict(T=0), dict(N=-3), dict(idx=None), dict(count=None), dict(flags=None)):
        _refused(L, L.gvec_traj_compact, _ptrs(TrajCompactArgs, **{**dict(T=8, N=4), **bad}))
    _refused(L, L.gvec_traj_compact, None)
    gat = dict(T=8, N=4, M=16, obs_floats=2025, mask_bytes=1125)
    for bad in (dict(T=0), dict(N=0), dict(M=-1), dict(obs_floats=0), dict(pos=None), dict(out_obs=None), dict(rejected=None), dict(mask=None)):
        _refused(L, L.gvec_traj_gather, _ptrs(TrajGatherArgs, **{**gat, **bad}))
    _refused(L, L.gvec_traj_gather, None)


def test_empty_gather_needs_no_device(L):
    from generalsreinforcementlearning_amd._lib import TrajGatherArgs
    a = TrajGatherArgs(T=8, N=4, M=0, obs_floats=2025, mask_bytes=1125)      # every pointer NULL
    assert L.gvec_traj_gather(0, None, C.byref(a)) == 0
    assert L.gvec_traj_scratch_bytes(128, 8192) >= 3 * 8 * 128 and L.gvec_traj_scratch_bytes(0, 4) == 0
