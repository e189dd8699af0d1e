"""The masked Q targets on the device (gvec_qtarget.hip through q_targets.py) against tests/_qtarget_reference.py, and the
recomputed mask against the env's own.

Mask and scalar target are defined to the bit and compared so.  The categorical target is compared with the float64
reference within tol = 8 x max|m_float32_ref - m_float64_ref| on the test's own inputs: the float32 reference's own error,
with a margin of 8 for the device's expf and its butterfly summation order, which differ from numpy's.  A row whose best
and second-best legal Q differ by less than 1e-3 in float64 may pick the other action in float32: such rows (at most 1 % of
a case) are held to a weaker bar - a finite, normalised m and a next_action among the reference's top two."""
import functools

import numpy as np
import pytest

import _qtarget_reference as R

pytestmark = pytest.mark.gpu

ROWS = 257                                           # no multiple of the kernels' four rows per workgroup
BOARDS = [(1, 1), (1, 7), (7, 5), (15, 15), (32, 32)]  # W x H; 15x15: H*W no multiple of 64; 32x32: the largest legal set
PAD = 13                                             # floats between two observations beyond 9 * H * W
V_MIN, V_MAX = -10.0, 10.0
NEAR_TIE = 1e-3
FULL_ROW, BARE_ROW = 5, 6                            # every tile owned and no mountain; no own tile


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _up(x):
    return _torch().from_numpy(np.array(x)).to(_dev())                  # a copy: the shared cases are read-only


@functools.lru_cache(maxsize=None)
def _case(W, H):
    """synthetic observations [ROWS, 9, H, W] of every row kind, their reference mask, rewards, discounts and done flags;
    computed once, shared, read-only"""
    rng = np.random.default_rng(1000 * W + H)
    n = W * H
    p_own = min(0.6, 12.0 / n)
    owner = rng.choice([0.0, 0.5, 1.0], (ROWS, n), p=[1 - 2 * p_own, p_own, p_own] if p_own <= 0.5 else [0.0, p_own, 1 - p_own])
    army = rng.choice([0, 1, 2, 3, 50, 4000], (ROWS, n), p=[0.1, 0.2, 0.2, 0.2, 0.2, 0.1])
    mtn = rng.random((ROWS, n)) < 0.15
    owner[FULL_ROW], mtn[FULL_ROW] = 0.5, False
    army[FULL_ROW] = rng.choice([2, 3, 50], n)
    owner[BARE_ROW] = rng.choice([0.0, 1.0], n)
    owner[mtn] = 0.0
    obs = rng.random((ROWS, 9, n)).astype(np.float32)                   # the planes the kernels must not read: anything
    obs[:, 1] = owner
    obs[:, 2] = np.where(owner > 0, np.log(army + 1) / 10.0, 0.0)
    obs[:, 4] = mtn
    obs = obs.reshape(ROWS, 9, H, W)
    mask = R.mask_from_observation(obs)
    reward = (3 * rng.standard_normal(ROWS)).astype(np.float32)
    reward[:8] = (-250.0, 250.0, -10.0, 10.0, 0.0, 1.5, -100.0, 100.0)   # beyond the support's bounds, and on them
    disc = rng.choice(np.float32([0.99, 0.9801, 0.970299, 0.5, 0.0]), ROWS)
    done = rng.random(ROWS) < 0.2
    done[[FULL_ROW, BARE_ROW]] = False
    for a in (obs, mask, reward, disc, done):
        a.setflags(write=False)
    return obs, mask, reward, disc, done


def _strided(obs):
    """the observations as rows of a wider CUDA tensor (NaN between them): read in place with obs_row_stride > 9 * H * W"""
    t = _torch()
    rows, _, H, W = obs.shape
    wide = t.full((rows, 9 * H * W + PAD), float("nan"), device=_dev())
    wide[:, :9 * H * W] = _up(obs.reshape(rows, -1))
    view = wide[:, :9 * H * W].view(rows, 9, H, W)
    assert not view.is_contiguous()
    return view


def _garbage(rng, values, mask):
    """NaN and +-1e30 at every illegal entry: they must change nothing"""
    junk = rng.choice(np.float32([np.nan, 1e30, -1e30]), mask.shape)
    shape = mask.shape + (1,) * (values.ndim - mask.ndim)
    return np.where(mask.reshape(shape), values, junk.reshape(shape)).astype(np.float32)


@pytest.mark.parametrize("W,H", BOARDS, ids=[f"{w}x{h}" for w, h in BOARDS])
def test_mask_of_synthetic_observations(W, H):
    from generalsreinforcementlearning_amd import valid_actions_mask_from_observation
    t = _torch()
    obs, mask, *_ = _case(W, H)
    assert not mask[BARE_ROW].any() and (W * H == 1 or mask[FULL_ROW].reshape(-1, 5)[:, 4].all())
    got = valid_actions_mask_from_observation(_up(obs))
    assert got.dtype == t.bool and tuple(got.shape) == (ROWS, 5 * W * H)
    assert np.array_equal(got.cpu().numpy(), mask)
    assert np.array_equal(valid_actions_mask_from_observation(_strided(obs)).cpu().numpy(), mask)
    out = t.full((ROWS, 5 * W * H), 7, dtype=t.uint8, device=_dev())                   # every byte is written, as 0 or 1
    ret = valid_actions_mask_from_observation(_up(obs), out=out)
    assert ret.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), mask.astype(np.uint8))
    lead = valid_actions_mask_from_observation(_up(obs[:256].reshape(4, 64, 9, H, W)))
    assert np.array_equal(lead.cpu().numpy(), mask[:256].reshape(4, 64, -1))
    # rows one at a time start at every alignment of 5 * H * W bytes
    flat = t.zeros(ROWS * 5 * W * H + 3, dtype=t.uint8, device=_dev())
    for off in (1, 2, 3):
        valid_actions_mask_from_observation(_up(obs), out=flat[off:off + ROWS * 5 * W * H])
        assert np.array_equal(flat[off:off + ROWS * 5 * W * H].cpu().numpy().reshape(ROWS, -1), mask.astype(np.uint8))


@pytest.mark.parametrize("per_row_discount", [True, False], ids=["discounts", "gamma"])
@pytest.mark.parametrize("double", [True, False], ids=["double", "single"])
@pytest.mark.parametrize("W,H", BOARDS, ids=[f"{w}x{h}" for w, h in BOARDS])
def test_scalar_target_is_bit_exact(W, H, double, per_row_discount):
    from generalsreinforcementlearning_amd import double_q_target
    obs, mask, reward, disc, done = _case(W, H)
    rng = np.random.default_rng(7)
    A = 5 * W * H
    q_eval = rng.standard_normal((ROWS, A)).astype(np.float32)
    q_sel = np.round(rng.standard_normal((ROWS, A)) * 4).astype(np.float32) / 4 if double else None    # quarter steps: ties
    if double:
        q_sel[10][mask[10]] = -np.inf                                                   # an all -inf legal set: its lowest index
        q_sel[11][mask[11]] = np.nan                                                    # NaN never wins: nothing does
        q_sel[12, np.flatnonzero(mask[12])[::2]] = np.nan
    q_eval, q_sel = _garbage(rng, q_eval, mask), (_garbage(rng, q_sel, mask) if double else None)
    discount = disc if per_row_discount else 0.97
    want_t, want_a, want_v = R.q_target(obs, q_eval, reward, discount, done, q_select=q_sel)
    assert (want_a[~mask.any(1)] == -1).all() and (not double or want_a[11] == -1)
    args = (_strided(obs), _up(q_eval), _up(reward), _up(disc) if per_row_discount else 0.97, _up(done))
    kw = dict(q_select=_up(q_sel) if double else None, return_next_value=True)
    got = [x.cpu().numpy() for x in double_q_target(*args, **kw)]
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want_a)
    assert np.array_equal(got[2].view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(got[0].view(np.uint32), want_t.view(np.uint32))
    again = [x.cpu().numpy() for x in double_q_target(*args, **kw)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
    two = double_q_target(args[0], args[1], _up(reward.astype(np.float64)), args[3], _up(done.astype(np.uint8)), q_select=kw["q_select"])
    assert len(two) == 2 and np.array_equal(two[0].cpu().numpy().view(np.uint32), want_t.view(np.uint32))


CATEGORICAL = [(1, 1, 2), (1, 7, 51), (7, 5, 64), (15, 15, 2), (15, 15, 51), (15, 15, 64), (32, 32, 2)]
# The first seed from 1 up for which the float64 reference finds at most 1 % of the rows of every case below within NEAR_TIE of
# a tie (2 of 257 rows; seeds 1 and 2 give one case 3): a property of the inputs and the reference alone, worked out on the CPU.
LOGIT_SEED = 3


@pytest.mark.parametrize("double", [True, False], ids=["double_discounts", "single_gamma"])
@pytest.mark.parametrize("W,H,N", CATEGORICAL, ids=[f"{w}x{h}_{n}atoms" for w, h, n in CATEGORICAL])
def test_categorical_target(W, H, N, double):
    """double: a selection network and per-row discounts; single: neither (logits_select NULL, the scalar gamma)"""
    from generalsreinforcementlearning_amd import categorical_target
    obs, mask, reward, disc, done = _case(W, H)
    rng = np.random.default_rng(LOGIT_SEED)
    A = 5 * W * H
    lg_eval = _garbage(rng, 2 * rng.standard_normal((ROWS, A, N), dtype=np.float32), mask)
    lg_sel = _garbage(rng, 2 * rng.standard_normal((ROWS, A, N), dtype=np.float32), mask) if double else None
    discount = disc if double else 0.97
    ref = dict(logits_select=lg_sel)
    m64, a64 = R.categorical_target(obs, lg_eval, reward, discount, done, V_MIN, V_MAX, dtype=np.float64, **ref)
    m32, a32 = R.categorical_target(obs, lg_eval, reward, discount, done, V_MIN, V_MAX, dtype=np.float32, **ref)
    # near ties, from the float64 reference alone
    q64 = R.categorical_q(obs, lg_eval if lg_sel is None else lg_sel, V_MIN, V_MAX)[0]
    order = np.argsort(-q64, axis=1, kind="stable")[:, :2]
    top = np.take_along_axis(q64, order, 1)
    with np.errstate(invalid="ignore"):                                              # -inf - -inf: a row without two legal actions
        near = ~done & np.isfinite(top[:, 1]) & (top[:, 0] - top[:, 1] < NEAR_TIE)
    print(f"{W}x{H} N={N}: {near.sum()} of {ROWS} rows within {NEAR_TIE} of a tie")
    assert near.mean() <= 0.01
    firm = ~near
    assert np.array_equal(a32[firm], a64[firm])
    tol = 8 * np.abs(m32[firm].astype(np.float64) - m64[firm]).max()
    assert tol < 1e-4

    args = (_strided(obs), _up(lg_eval), _up(reward), _up(disc) if double else 0.97, _up(done), V_MIN, V_MAX)
    kw = dict(logits_select=_up(lg_sel) if double else None)
    m, a = (x.cpu().numpy() for x in categorical_target(*args, **kw))
    assert m.dtype == np.float32 and m.shape == (ROWS, N) and a.dtype == np.int64
    err = np.abs(m[firm].astype(np.float64) - m64[firm]).max()
    print(f"{W}x{H} N={N}: max |m - m_float64| = {err:.3g}, tol = {tol:.3g}, float32 reference {tol / 8:.3g}")
    assert np.isfinite(m).all() and (m >= 0).all()
    assert np.abs(m.astype(np.float64).sum(1) - 1).max() <= 1e-5
    assert np.array_equal(a[firm], a64[firm])
    assert (a[done] == -1).all() and (a[~mask.any(1)] == -1).all()
    assert err <= tol
    for i in np.flatnonzero(near):
        assert a[i] in order[i]
    m2, a2 = (x.cpu().numpy() for x in categorical_target(*args, **kw))
    assert np.array_equal(m.view(np.uint32), m2.view(np.uint32)) and np.array_equal(a, a2)


FORMS = [(1, 1), (5, 6), (32, 32)]                   # W x H


@pytest.mark.parametrize("W,H", FORMS, ids=[f"{w}x{h}" for w, h in FORMS])
def test_python_front_reads_every_form_of_a_batch(W, H):
    """six observations, handed over in every form the three functions accept: the reference's mask and targets, row by row,
    whichever way the rows reach the kernels.  Mask and scalar target to the bit; the categorical target under the rule of
    test_categorical_target (tol = 8 x the float32 reference's own error on these rows, rows near a tie left out)."""
    from generalsreinforcementlearning_amd import categorical_target, double_q_target, valid_actions_mask_from_observation
    from generalsreinforcementlearning_amd._obs_batch import in_place
    t = _torch()
    obs, mask, reward, disc, done = (a[:6] for a in _case(W, H))
    rng = np.random.default_rng(11)
    A, N, n, nan = 5 * W * H, 5, 9 * W * H, float("nan")
    q_eval, q_sel = (_garbage(rng, rng.standard_normal((6, A)).astype(np.float32), mask) for _ in range(2))
    lg_eval, lg_sel = (_garbage(rng, 2 * rng.standard_normal((6, A, N), dtype=np.float32), mask) for _ in range(2))
    want_t, want_a, _ = R.q_target(obs, q_eval, reward, disc, done, q_select=q_sel)
    m64, a64 = R.categorical_target(obs, lg_eval, reward, disc, done, V_MIN, V_MAX, logits_select=lg_sel, dtype=np.float64)
    m32, _ = R.categorical_target(obs, lg_eval, reward, disc, done, V_MIN, V_MAX, logits_select=lg_sel, dtype=np.float32)
    top = -np.sort(-R.categorical_q(obs, lg_sel, V_MIN, V_MAX)[0], axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        firm = ~(~done & np.isfinite(top[:, -1]) & (top[:, 0] - top[:, -1] < NEAR_TIE))
    assert firm.sum() >= 5
    tol = 8 * np.abs(m32[firm].astype(np.float64) - m64[firm]).max()
    assert tol < 1e-4

    x = _up(obs)
    wide = t.full((6, n + PAD), nan, device=_dev())
    wide[:, :n] = x.view(6, n)
    strided = wide[:, :n].view(6, 9, H, W)
    read, stride = in_place(strided, 3, H, W)
    assert not strided.is_contiguous() and read.data_ptr() == strided.data_ptr() and stride == n + PAD     # read where they are
    gappy = t.full((2, 4, 9, H, W), nan, device=_dev())
    gappy[:, :3] = x.view(2, 3, 9, H, W)
    assert in_place(gappy[:, :3], 3, H, W)[0].data_ptr() != gappy.data_ptr()                              # no common stride: copied
    forms = [(x.view(2, 3, 9, H, W), (2, 3), np.arange(6)), (x[0], (), np.array([0])), (strided, (6,), np.arange(6)),
             (gappy[:, :3], (2, 3), np.arange(6)), (x[:1].expand(6, 9, H, W), (6,), np.zeros(6, np.int64)),
             (x[:0].view(0, 3, 9, H, W), (0, 3), np.arange(0))]
    for o, lead, idx in forms:
        per_row = lambda a: _up(a[idx].reshape(lead + a.shape[1:]))
        got = valid_actions_mask_from_observation(o)
        assert got.dtype == t.bool and tuple(got.shape) == lead + (A,)
        assert np.array_equal(got.cpu().numpy().reshape(len(idx), A), mask[idx])
        tq, act = double_q_target(o, per_row(q_eval), per_row(reward), per_row(disc), per_row(done), q_select=per_row(q_sel))
        assert tuple(tq.shape) == lead == tuple(act.shape) and np.array_equal(act.cpu().numpy().reshape(-1), want_a[idx])
        assert np.array_equal(tq.cpu().numpy().reshape(-1).view(np.uint32), want_t[idx].view(np.uint32))
        m, act = categorical_target(o, per_row(lg_eval), per_row(reward), per_row(disc), per_row(done), V_MIN, V_MAX,
                                    logits_select=per_row(lg_sel))
        assert tuple(m.shape) == lead + (N,) and tuple(act.shape) == lead
        m, act, keep = m.cpu().numpy().reshape(len(idx), N), act.cpu().numpy().reshape(-1), firm[idx]
        assert np.array_equal(act[keep], a64[idx][keep]) and np.isfinite(m).all()
        if keep.any():
            err = np.abs(m[keep].astype(np.float64) - m64[idx][keep]).max()
            print(f"{W}x{H} lead {lead}: max |m - m_float64| = {err:.3g}, tol = {tol:.3g}")
            assert err <= tol
    assert bool(wide[:, n:].isnan().all())
    for dtype in (t.bool, t.uint8):                                                     # out=, both dtypes: every byte written
        out = t.ones(6 * A, dtype=dtype, device=_dev())
        ret = valid_actions_mask_from_observation(x.view(2, 3, 9, H, W), out=out)
        assert ret.data_ptr() == out.data_ptr() and ret.dtype == t.bool and tuple(ret.shape) == (2, 3, A)
        assert np.array_equal(out.view(t.uint8).cpu().numpy().reshape(6, A), mask.astype(np.uint8))


def _random_legal(t, mask, gen):
    """one legal action per row of a bool mask [..., A] (0 where a row has none)"""
    m = mask.reshape(-1, mask.shape[-1]).float()
    m[m.sum(1) == 0, 0] = 1.0
    return t.multinomial(m, 1, generator=gen).squeeze(1).reshape(mask.shape[:-1])


@pytest.mark.parametrize("kind", ["single", "selfplay"])
def test_mask_equals_the_envs_own_at_every_step(kind):
    """60 masked-random steps: the mask recomputed from the observation is info["valid_actions_mask"], for every learner's row"""
    from generalsreinforcementlearning_amd import valid_actions_mask_from_observation
    t = _torch()
    if kind == "single":
        from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
        env = GeneralsVecEnv(64, board_width=8, board_height=8, device_outputs=True, seed=3)
    else:
        from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
        env = GeneralsSelfPlayVecEnv(32, 15, 15, max_players=4, device_outputs=True, seed=3)
    gen = t.Generator(device=_dev())
    gen.manual_seed(11)
    try:
        obs, info = env.reset()
        legal = 0
        for step in range(61):
            want = info["valid_actions_mask"]
            got = valid_actions_mask_from_observation(obs)
            assert got.shape == want.shape
            assert t.equal(got.view(t.uint8), want.view(t.uint8) if want.dtype == t.bool else want), (kind, step)
            legal += int(want.sum())
            obs, _, _, _, info = env.step(_random_legal(t, want.bool(), gen))
        assert legal > 0
    finally:
        env.close()
