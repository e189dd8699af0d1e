"""The fog-of-war memory planes on the GPU (gvec_obs_memory_update, memory.ObservationMemory, SelfPlayRolloutBuffer's memory=)
against the numpy restatement of tests/_memory_reference.py.

cap is a power of two, so every age is an exact float32 whatever computes it, and owner and army are copied: every comparison
is np.array_equal.  There is no tolerance.  A sequence is uploaded once, its updates write the slots of one device tensor and
that is read back once.

What the random sequences cannot reach: with a tile visible three steps in ten, one that stays hidden for 64 steps in a row
does not occur, so among them only cap = 2 saturates an age with seen = 1.  test_age_saturates_at_every_cap drives that edge
at cap 64 (and short of it at 1,024) directly."""
import ctypes as C
import functools

import numpy as np
import pytest

import _memory_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(5, 5), (8, 8), (15, 15), (20, 20), (32, 32), (32, 3), (3, 32)]     # W x H
ROWS = [(1, 1), (3, 1), (67, 1), (4, 2), (68, 2), (4, 4), (68, 4)]            # (rows, rows_per_flag)
CAPS = [2, 64, 1024]
STEPS = 70                                                                    # past cap 64


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _up(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).to(_dev())


def hip_update(obs, prev, reset, out, W, H, cap, rows, rows_per_flag=1, stride=None):
    """the C entry point on device tensors: obs / prev / out any float32 tensors whose data_ptr() is row 0"""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import ObsMemoryArgs, check
    t = _torch()
    a = ObsMemoryArgs(rows=rows, width=W, height=H, cap=cap, rows_per_flag=rows_per_flag, obs_row_stride=9 * W * H if stride is None else stride,
                      obs=obs.data_ptr(), prev=None if prev is None else prev.data_ptr(), reset=None if reset is None else reset.data_ptr(),
                      out=out.data_ptr())
    check(g.load().gvec_obs_memory_update(0, t.cuda.current_stream(_dev()).cuda_stream, C.byref(a)), "gvec_obs_memory_update")
    return out


@functools.lru_cache(maxsize=2)                                               # 175 MB at 68 rows of 32x32: not kept for the session
def _sequence(W, H, rows, rpf):
    """(obs [STEPS, rows, 9, H, W], reset [STEPS, rows / rpf]) - drawn once, left unchanged"""
    rng = np.random.default_rng(100000 * W + 1000 * H + 10 * rows + rpf)
    obs, reset = R.random_sequence(rng, STEPS, rows, H, W, rows_per_flag=rpf)
    obs.setflags(write=False)
    reset.setflags(write=False)
    return obs, reset


@functools.lru_cache(maxsize=4)
def _reference(W, H, rows, rpf, cap):
    obs, reset = _sequence(W, H, rows, rpf)
    ref = R.run(obs, reset, cap, rpf)
    ref.setflags(write=False)
    return ref


def _run_hip(d_obs, d_reset, W, H, cap, rows, rpf, in_place=False):
    """every step's state [STEPS, rows, 4, H, W] from the kernel, given the sequence on the device; out of place each update
    reads slot s - 1 and writes slot s"""
    t = _torch()
    store = t.full((STEPS, rows, 4, H, W), np.nan, dtype=t.float32, device=_dev())
    state = None
    for s in range(STEPS):
        if in_place:
            if state is None:
                state = _up(R.blank(rows, H, W))
            hip_update(d_obs[s], state, d_reset[s], state, W, H, cap, rows, rpf)
            store[s].copy_(state)
        else:
            hip_update(d_obs[s], None if s == 0 else store[s - 1], d_reset[s], store[s], W, H, cap, rows, rpf)
    return store.cpu().numpy()


def _check_identities(obs, got):
    """the two identities of the definition, on every step"""
    vis = obs[:, :, 0] != 0
    assert np.array_equal(got[:, :, R.LAST_OWNER][vis], obs[:, :, 1][vis]) and np.array_equal(got[:, :, R.LAST_ARMY][vis], obs[:, :, 2][vis])
    assert (got[:, :, R.SEEN][vis] == 1.0).all() and (got[:, :, R.AGE][vis] == 0.0).all()
    assert (obs[:, :, 1][~vis] == 0.0).all() and (obs[:, :, 2][~vis] == 0.0).all()
    # so planes 1 and 2 of the memory are the observation's wherever it shows something, and remember where it shows nothing
    shown = np.where(vis[:, :, None], obs[:, :, 1:3], got[:, :, 1:3])
    assert np.array_equal(got[:, :, 1:3].view(np.uint32), shown.view(np.uint32))


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_bit_exact_against_the_reference(W, H):
    aging = saturated = restarted = False
    for rows, rpf in ROWS:
        obs, reset = _sequence(W, H, rows, rpf)
        d_obs, d_reset = _up(obs), _up(reset)
        for cap in CAPS:
            want = _reference(W, H, rows, rpf, cap)
            got = _run_hip(d_obs, d_reset, W, H, cap, rows, rpf)
            assert not np.isnan(got).any(), "an element was not written"
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, rpf, cap, np.argwhere(got != want)[:8])
            _check_identities(obs, got)
            # the inputs are not vacuous, read off the reference's own output
            age, seen = want[:, :, R.AGE], want[:, :, R.SEEN]
            aging |= bool(((age > 0) & (age < 1)).any())
            saturated |= bool(((age == 1) & (seen == 1)).any())
            had_seen = seen[:-1].reshape(STEPS - 1, rows, -1).any(axis=2)
            restarted |= bool((had_seen & (np.repeat(reset[1:], rpf, axis=1) != 0)).any())
    assert aging, "no tile with 0 < age < 1"
    assert saturated, "no tile with age == 1 and seen == 1"
    assert restarted, "no row was reset after having seen something"


@pytest.mark.parametrize("W,H,rows,rpf,cap", [(15, 15, 67, 1, 64), (20, 20, 68, 4, 2), (5, 5, 3, 1, 1024)])
def test_in_place_equals_out_of_place(W, H, rows, rpf, cap):
    obs, reset = _sequence(W, H, rows, rpf)
    got = _run_hip(_up(obs), _up(reset), W, H, cap, rows, rpf, in_place=True)
    want = _reference(W, H, rows, rpf, cap)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_age_saturates_at_every_cap():
    """a tile seen once and hidden for 69 updates: age k / cap until it reaches 1.0, where it stays with seen = 1"""
    t = _torch()
    W, H, rows = 8, 8, 3
    obs = np.zeros((STEPS, rows, 9, H, W), np.float32)
    obs[0, :, 0], obs[0, :, 1], obs[0, :, 2] = 1.0, 1.0, np.float32(0.25)
    obs[:, 2, 0, 0, 0] = 1.0                                             # one tile of row 2 stays in sight
    for cap in CAPS:
        want = R.run(obs, None, cap)
        store = t.full((STEPS, rows, 4, H, W), np.nan, dtype=t.float32, device=_dev())
        d_obs = _up(obs)
        for s in range(STEPS):
            hip_update(d_obs[s], None if s == 0 else store[s - 1], None, store[s], W, H, cap, rows)
        got = store.cpu().numpy()
        assert np.array_equal(got, want)
        assert [float(v) for v in got[:, 0, R.AGE, 3, 3]] == [min(k, cap) / cap for k in range(STEPS)]
        assert (got[:, 0, R.SEEN] == 1.0).all() and (got[:, 0, R.LAST_ARMY] == np.float32(0.25)).all()
        assert (got[:, 2, R.AGE, 0, 0] == 0.0).all()
        assert (got[-1, 0, R.AGE] == (1.0 if cap <= 64 else 69 / 1024)).all()


def test_null_prev_is_a_blank_prev_and_null_reset_is_no_flag():
    t = _torch()
    W, H, rows, rpf, cap = 15, 15, 68, 2, 64
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    d_obs = _up(obs[11])
    new = lambda: t.full((rows, 4, H, W), np.nan, dtype=t.float32, device=_dev())
    from_null = hip_update(d_obs, None, None, new(), W, H, cap, rows, rpf)
    from_blank = hip_update(d_obs, _up(R.blank(rows, H, W)), None, new(), W, H, cap, rows, rpf)
    assert t.equal(from_null.view(t.int32), from_blank.view(t.int32))
    assert np.array_equal(from_null.cpu().numpy(), R.update(None, obs[11], None, cap))
    # all flags set: a blank start again, whatever prev holds
    all_set = hip_update(d_obs, _up(ref[10]), t.ones(rows // rpf, dtype=t.uint8, device=_dev()), new(), W, H, cap, rows, rpf)
    assert t.equal(all_set.view(t.int32), from_null.view(t.int32))
    prev = _up(ref[10])
    no_flags = hip_update(d_obs, prev, None, new(), W, H, cap, rows, rpf)
    zero_flags = hip_update(d_obs, prev, t.zeros(rows // rpf, dtype=t.uint8, device=_dev()), new(), W, H, cap, rows, rpf)
    assert t.equal(no_flags.view(t.int32), zero_flags.view(t.int32))
    assert np.array_equal(no_flags.cpu().numpy(), R.update(ref[10], obs[11], None, cap))
    assert not t.equal(no_flags, from_null)


def test_row_stride_unread_planes_and_untouched_inputs():
    t = _torch()
    W, H, rows, rpf, cap, gap = 15, 15, 67, 1, 64, 13
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    n = 9 * W * H
    big = t.full((rows, n + gap), 7.25, dtype=t.float32, device=_dev())
    big[:, :n] = _up(obs[21].reshape(rows, n))
    big[:, 3 * W * H:n] = float("nan")                                   # planes 3 to 8 are not read
    before, prev = big.clone(), _up(ref[20])
    prev_before = prev.clone()
    out = t.full((rows, 4, H, W), np.nan, dtype=t.float32, device=_dev())
    hip_update(big, prev, _up(reset[21]), out, W, H, cap, rows, rpf, stride=n + gap)
    assert np.array_equal(out.cpu().numpy(), ref[21])
    assert t.equal(big.view(t.int32), before.view(t.int32)) and t.equal(prev, prev_before)
    # the Python front reads the same view in place
    from generalsreinforcementlearning_amd import ObservationMemory
    view = big[:, :n].view(rows, 9, H, W)
    assert not view.is_contiguous()
    m = ObservationMemory((rows,), H, W, cap=cap)
    m.load_state_dict({"planes": prev, "cap": cap, "rows_shape": (rows,), "height": H, "width": W})
    assert np.array_equal(m.update(view, _up(reset[21])).cpu().numpy(), ref[21])


@pytest.mark.parametrize("W,H", [(15, 15), (20, 20), (5, 5)], ids=["15x15", "20x20", "5x5"])
def test_base_pointers_off_16_byte_alignment(W, H):
    t = _torch()
    rows, rpf, cap = 3, 1, 64
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    n_obs, n_mem = rows * 9 * W * H, rows * 4 * W * H
    d_reset = _up(reset[31])
    for off_obs in range(4):
        for off_prev in range(4):
            for off_out in range(4):
                src = t.zeros(n_obs + 8, dtype=t.float32, device=_dev())
                src[off_obs:off_obs + n_obs] = _up(obs[31].reshape(-1))
                prev = t.zeros(n_mem + 8, dtype=t.float32, device=_dev())
                prev[off_prev:off_prev + n_mem] = _up(ref[30].reshape(-1))
                dst = t.full((n_mem + 4 + 16,), -3.5, dtype=t.float32, device=_dev())
                assert src.data_ptr() % 16 == 0 and prev.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
                hip_update(src[off_obs:], prev[off_prev:], d_reset, dst[off_out:], W, H, cap, rows, rpf)
                d = dst.cpu().numpy()
                where = (off_obs, off_prev, off_out)
                assert np.array_equal(d[off_out:off_out + n_mem].reshape(rows, 4, H, W), ref[31]), where
                assert (d[:off_out] == -3.5).all() and (d[off_out + n_mem:] == -3.5).all(), where    # the sentinel behind out's end
    # in place at an odd offset
    state = t.full((n_mem + 4 + 16,), -3.5, dtype=t.float32, device=_dev())
    state[3:3 + n_mem] = _up(ref[30].reshape(-1))
    hip_update(_up(obs[31]), state[3:], d_reset, state[3:], W, H, cap, rows, rpf)
    d = state.cpu().numpy()
    assert np.array_equal(d[3:3 + n_mem].reshape(rows, 4, H, W), ref[31]) and (d[:3] == -3.5).all() and (d[3 + n_mem:] == -3.5).all()


# ---- the Python class ------------------------------------------------------------------------------------------------

def test_python_front_state_and_outputs():
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory
    W, H, rows, rpf, cap = 8, 8, 68, 4, 64
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    B, L = rows // rpf, rpf
    m = ObservationMemory((B, L), H, W, cap=cap)
    assert np.array_equal(m.planes.cpu().numpy().reshape(rows, 4, H, W), R.blank(rows, H, W))
    d_obs = _up(obs).view(STEPS, B, L, 9, H, W).requires_grad_(True)
    slots = t.full((4, rows * 4 * H * W), np.nan, dtype=t.float32, device=_dev())
    for s in range(12):
        flags = _up(reset[s]) if s % 2 else _up(reset[s]).bool()         # uint8 and bool alike
        if s < 6:
            p = m.update(d_obs[s], flags)                                # in place
            assert s == 0 or p.data_ptr() == ptr
            ptr = p.data_ptr()
        else:
            p = m.update(d_obs[s], flags, out=slots[s % 4])              # into a slot: the state lives there afterwards
            assert p.data_ptr() == slots[s % 4].data_ptr() == m.planes.data_ptr()
        assert p.shape == (B, L, 4, H, W) and not p.requires_grad
        assert np.array_equal(p.cpu().numpy().reshape(rows, 4, H, W), ref[s]), s
    assert np.array_equal(slots[2].cpu().numpy().reshape(rows, 4, H, W), ref[10])    # an earlier slot keeps its step
    m.reset_all()
    assert np.array_equal(m.planes.cpu().numpy().reshape(rows, 4, H, W), R.blank(rows, H, W))
    m.reset_all()
    assert np.array_equal(m.update(d_obs[5].detach()).cpu().numpy().reshape(rows, 4, H, W), R.update(None, obs[5], None, cap))
    # rows that share no common stride are copied first: same result
    wide = t.zeros((2 * B, L, 9, H, W), dtype=t.float32, device=_dev())
    wide[::2] = d_obs[6].detach()
    m.load_state_dict({"planes": _up(ref[5]).view(B, L, 4, H, W), "cap": cap, "rows_shape": (B, L), "height": H, "width": W})
    assert np.array_equal(m.update(wide[::2], _up(reset[6])).cpu().numpy().reshape(rows, 4, H, W), ref[6])
    with pytest.raises(ValueError):
        m.update(d_obs[0].detach(), out=t.empty(5, dtype=t.float32, device=_dev()))
    with pytest.raises(ValueError):
        m.update(d_obs[0].detach(), reset=t.zeros(B, dtype=t.bool))      # flags on the host
    empty = ObservationMemory((0, 2), H, W)
    assert empty.update(t.zeros((0, 2, 9, H, W), dtype=t.float32, device=_dev())).shape == (0, 2, 4, H, W)


def test_copy_envs_and_state_dict():
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory
    W, H, rows, rpf, cap = 8, 8, 68, 4, 64
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    B, L = rows // rpf, rpf
    m = ObservationMemory((B, L), H, W, cap=cap)
    m.load_state_dict({"planes": _up(ref[20]).view(B, L, 4, H, W), "cap": cap, "rows_shape": (B, L), "height": H, "width": W})
    before = m.planes.clone()
    m.copy_envs([9, 10, 16], t.tensor([0, 1, 1], device=_dev()))         # a source may repeat
    after = m.planes
    want = before.clone()
    want[9], want[10], want[16] = before[0], before[1], before[1]
    assert t.equal(after.view(t.int32), want.view(t.int32))              # the copied rows, and the others bit-identical
    assert not t.equal(after[9], before[9])
    with pytest.raises(ValueError):
        m.copy_envs([1, 2], [3])
    saved = m.state_dict()
    m.update(_up(obs[21]).view(B, L, 9, H, W), _up(reset[21]))
    assert not t.equal(m.planes, saved["planes"])                        # the saved planes are a copy
    assert t.equal(saved["planes"].view(t.int32), want.view(t.int32))
    other = ObservationMemory((B, L), H, W, cap=cap)
    other.load_state_dict(saved)
    assert t.equal(other.planes.view(t.int32), want.view(t.int32))
    nxt = R.update(want.cpu().numpy().reshape(rows, 4, H, W), obs[22], reset[22], cap, rpf)
    assert np.array_equal(other.update(_up(obs[22]).view(B, L, 9, H, W), _up(reset[22])).cpu().numpy().reshape(rows, 4, H, W), nxt)
    for bad in (dict(saved, cap=32), dict(saved, rows_shape=(B * L,)), dict(saved, planes=saved["planes"][:, :1])):
        with pytest.raises(ValueError):
            other.load_state_dict(bad)


FORMS = [(1, 1), (5, 6), (32, 32)]                                       # W x H


@pytest.mark.parametrize("W,H", FORMS, ids=[f"{w}x{h}" for w, h in FORMS])
def test_python_front_reads_every_form_of_a_batch(W, H):
    """the second of two observations of six rows, handed over in every form update accepts: the reference's state whichever way
    the rows reach the kernel"""
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory
    from generalsreinforcementlearning_amd._obs_batch import in_place
    cap, n, nan = 16, 9 * W * H, float("nan")
    obs, reset = R.random_sequence(np.random.default_rng(100 * W + H), 2, 6, H, W, rows_per_flag=3, p_reset=0.5)
    reset[1] = (1, 0)
    first = R.update(None, obs[0], None, cap)
    want = R.update(first, obs[1], None, cap)
    want_reset = R.update(first, obs[1], reset[1], cap, rows_per_flag=3)
    assert not np.array_equal(want, want_reset) or W * H == 1
    x0, x1 = _up(obs[0]), _up(obs[1])

    def after_first(rows_shape, src=x0):
        m = ObservationMemory(rows_shape, H, W, cap=cap)
        m.update(src.view(rows_shape + (9, H, W)))
        return m

    def same(planes, expected):
        return np.array_equal(planes.cpu().numpy().reshape(expected.shape).view(np.uint32), expected.view(np.uint32))

    p = after_first((2, 3)).update(x1.view(2, 3, 9, H, W), _up(reset[1]))                  # leading shape (2, 3), a flag per env
    assert p.shape == (2, 3, 4, H, W) and same(p, want_reset)
    p = after_first((), x0[0]).update(x1[0])                                                     # no leading shape
    assert p.shape == (4, H, W) and same(p, want[0])
    # rows of a wider tensor, NaN between them: read where they are
    wide = t.full((6, n + 13), nan, dtype=t.float32, device=_dev())
    wide[:, :n] = x1.view(6, n)
    view = wide[:, :n].view(6, 9, H, W)
    read, stride = in_place(view, 3, H, W)
    assert not view.is_contiguous() and read.data_ptr() == view.data_ptr() and stride == n + 13
    assert same(after_first((6,)).update(view), want) and bool(wide[:, n:].isnan().all())
    # three of every four rows: no common stride, copied
    gappy = t.full((2, 4, 9, H, W), nan, dtype=t.float32, device=_dev())
    gappy[:, :3] = x1.view(2, 3, 9, H, W)
    assert in_place(gappy[:, :3], 3, H, W)[0].data_ptr() != gappy.data_ptr()
    assert same(after_first((2, 3)).update(gappy[:, :3], _up(reset[1]).bool()), want_reset)
    # one observation expanded to six rows: stride 0, copied
    m = after_first((6,), x0[:1].expand(6, 9, H, W).contiguous())
    assert same(m.update(x1[:1].expand(6, 9, H, W)), np.repeat(want[:1], 6, axis=0))
    m, out = after_first((2, 3)), t.full((6 * 4 * H * W,), nan, dtype=t.float32, device=_dev())
    p = m.update(x1.view(2, 3, 9, H, W), out=out)
    assert p.data_ptr() == out.data_ptr() == m.planes.data_ptr() and same(out, want)
    empty = ObservationMemory((0, 3), H, W, cap=cap)
    assert empty.update(x1[:0].view(0, 3, 9, H, W), out=out[:0]).shape == (0, 3, 4, H, W)


# ---- a real env --------------------------------------------------------------------------------------------------------

def _random_legal(t, mask, gen):
    """one legal action per row of a bool mask [..., A] (0 where a row has none)"""
    m = mask.reshape(-1, mask.shape[-1]).float()
    m[m.sum(1) == 0, 0] = 1.0
    return t.multinomial(m, 1, generator=gen).squeeze(1).reshape(mask.shape[:-1])


ENV_SEED = 9        # of seeds 0-11 the one whose 40 random steps lose sight of the most enemy tiles (10 tile-steps; most seeds: none)


@pytest.mark.parametrize("fog", [True, False], ids=["fog", "no_fog"])
def test_on_a_self_play_env(fog):
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory, remembered_observation
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, W, H, L = 64, 8, 8, 2
    env = GeneralsSelfPlayVecEnv(B, W, H, max_players=2, max_turns=12, device_outputs=True, fog_of_war=fog, seed=ENV_SEED)
    gen = t.Generator(device=_dev())
    gen.manual_seed(5)
    m = ObservationMemory((B, L), H, W)
    try:
        obs, info = env.reset()
        want = R.update(None, obs.cpu().numpy().reshape(B * L, 9, H, W))
        got = m.update(obs)
        assert np.array_equal(got.cpu().numpy().reshape(B * L, 4, H, W), want)
        redealt, lost_sight_of_an_enemy = 0, 0
        for step in range(40):
            obs, _, _, _, info = env.step(_random_legal(t, info["valid_actions_mask"], gen))
            flags = info["reset"]
            h_obs = obs.cpu().numpy().reshape(B * L, 9, H, W)
            want = R.update(want, h_obs, flags.cpu().numpy(), rows_per_flag=L)
            got = m.update(obs, flags)
            h_got = got.cpu().numpy().reshape(B * L, 4, H, W)
            assert np.array_equal(h_got.view(np.uint32), want.view(np.uint32)), step
            hidden = h_obs[:, 0] == 0
            assert (h_obs[:, 1][hidden] == 0).all() and (h_obs[:, 2][hidden] == 0).all()   # what the second identity rests on
            r = remembered_observation(obs, got).cpu().numpy().reshape(B * L, 9, H, W)
            assert np.array_equal(r[:, 1:3], np.where(hidden[:, None], h_got[:, 1:3], h_obs[:, 1:3]))
            assert np.array_equal(r[:, 0], h_obs[:, 0]) and np.array_equal(r[:, 3:], h_obs[:, 3:])
            redealt += int(flags.sum())
            lost_sight_of_an_enemy += int((hidden & (h_got[:, R.LAST_OWNER] == 1.0)).sum())
            if not fog:
                assert not hidden.any() and (h_got[:, R.AGE] == 0.0).all() and (h_got[:, R.SEEN] == 1.0).all()
        print(f"fog {fog}: {redealt} re-deals, {lost_sight_of_an_enemy} hidden tiles remembered as somebody else's")
        assert redealt >= 1
        if fog:
            assert lost_sight_of_an_enemy >= 1
    finally:
        env.close()


def test_remembered_enemy_reaches_the_strategic_features():
    """an enemy tile visible at step 0 and fogged at step 1: the raw observation's distance plane goes blank, the remembered one's
    does not"""
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory, remembered_observation, strategic_features
    H = W = 8
    o0 = np.zeros((1, 9, H, W), np.float32)
    o0[0, 0, :3, :3] = 1.0                                               # the learner sees a 3x3 corner
    o0[0, 1, 0, 0], o0[0, 2, 0, 0], o0[0, 6, 0, 0] = 0.5, np.float32(np.log(6.0) / 10), 1.0     # its general
    o0[0, 1, 2, 2], o0[0, 2, 2, 2] = 1.0, np.float32(np.log(4.0) / 10)                          # an enemy tile at (2, 2)
    o1 = o0.copy()
    o1[0, 0, 2, 2] = o1[0, 1, 2, 2] = o1[0, 2, 2, 2] = 0.0               # the fog takes it back
    m = ObservationMemory((1,), H, W)
    m.update(_up(o0))
    d1 = _up(o1)
    mem = m.update(d1)
    raw = strategic_features(d1).cpu().numpy()[0]
    assert (raw[1] == 1.0).all()
    rem = strategic_features(remembered_observation(d1, mem)).cpu().numpy()[0]
    assert rem[1, 2, 2] == 0.0 and rem[1, 0, 0] == np.float32(4 / 64) and rem[1, 7, 7] == np.float32(10 / 64)
    h = mem.cpu().numpy()[0]
    assert h[R.LAST_OWNER, 2, 2] == 1.0 and h[R.AGE, 2, 2] == np.float32(1 / 64) and h[R.LAST_ARMY, 2, 2] == np.float32(np.log(4.0) / 10)


# ---- the rollout buffer ------------------------------------------------------------------------------------------------

def test_rollout_buffer_carries_the_memory():
    t = _torch()
    from generalsreinforcementlearning_amd import ObservationMemory, SelfPlayRolloutBuffer
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, W, H, L, T = 16, 8, 8, 2, 8
    N = B * L
    env = GeneralsSelfPlayVecEnv(B, W, H, max_players=2, max_turns=6, device_outputs=True, seed=ENV_SEED)
    gen = t.Generator(device=_dev())
    gen.manual_seed(7)
    try:
        mem = ObservationMemory((B, L), H, W)
        buf = SelfPlayRolloutBuffer(env, horizon=T, memory=mem)
        assert tuple(buf.mem_store.shape) == (T + 1, N, 4, H * W)
        buf.begin(*env.reset())
        want, resets = None, 0
        for rollout in range(2):
            flags = [None]
            while not buf.full:
                assert buf.memory.shape == (B, L, 4, H, W) and buf.memory.data_ptr() == mem.planes.data_ptr()
                a = _random_legal(t, buf.valid_actions_mask, gen)
                out = buf.step(a, t.zeros(B, L, device=_dev()), t.zeros(B, L, device=_dev()))
                flags.append(out[4]["reset"].cpu().numpy())
            h_obs = buf.obs_store.cpu().numpy().reshape(T + 1, N, 9, H, W)
            h_mem = buf.mem_store.cpu().numpy().reshape(T + 1, N, 4, H, W)
            for k in range(T + 1):
                if not (rollout and k == 0):                             # slot 0 of the second rollout is the old slot T
                    want = R.update(want, h_obs[k], flags[k], rows_per_flag=L)
                assert np.array_equal(h_mem[k].view(np.uint32), want.view(np.uint32)), (rollout, k)
                resets += 0 if flags[k] is None else int(flags[k].sum())
            buf.finish(t.zeros(B, L, device=_dev()))
            pos = t.tensor([0, 5, N - 1, N, 3 * N + 7, T * N - 1, 5], device=_dev())
            batch = buf.gather(pos)
            assert sorted(batch) == sorted(["obs", "valid_actions_mask", "action", "logp", "value", "returns", "advantages", "weight",
                                            "index", "memory"])
            assert batch["memory"].shape == (len(pos), 4, H, W)
            assert np.array_equal(batch["memory"].cpu().numpy(), h_mem.reshape(-1, 4, H, W)[pos.cpu().numpy()])
            rows = sum(int(b["memory"].shape[0]) for b in buf.minibatches(100, seed=1))
            assert rows == T * N
            b = next(iter(buf.minibatches(64, seed=2)))
            assert np.array_equal(b["memory"].cpu().numpy(), h_mem.reshape(-1, 4, H, W)[b["index"].cpu().numpy()])
            assert np.array_equal(b["obs"].cpu().numpy(), h_obs.reshape(-1, 9, H, W)[b["index"].cpu().numpy()])
            last = buf.mem_store[T].clone()
            buf.next_rollout()
            assert t.equal(buf.mem_store[0].view(t.int32), last.view(t.int32)) and buf.memory.data_ptr() == buf.mem_store[0].data_ptr()
            assert mem.planes.data_ptr() == buf.mem_store[0].data_ptr()
        assert resets >= 1                                               # max_turns < 2 T: re-deals went through the store
    finally:
        env.close()


def test_rollout_buffer_without_memory_is_what_it_was():
    t = _torch()
    from generalsreinforcementlearning_amd import SelfPlayRolloutBuffer
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, W, H, L, T = 16, 8, 8, 2, 8
    env = GeneralsSelfPlayVecEnv(B, W, H, max_players=2, max_turns=6, device_outputs=True, seed=ENV_SEED)
    try:
        buf = SelfPlayRolloutBuffer(env, horizon=T)
        assert buf.mem_store is None and buf.memory is None
        buf.begin(*env.reset())
        while not buf.full:
            buf.step(t.zeros(B, L, dtype=t.int64, device=_dev()), t.zeros(B, L, device=_dev()), t.zeros(B, L, device=_dev()))
        buf.finish(t.zeros(B, L, device=_dev()))
        today = ["action", "advantages", "index", "logp", "obs", "returns", "valid_actions_mask", "value", "weight"]
        assert sorted(buf.gather(t.arange(10, device=_dev()))) == today
        assert all(sorted(b) == today for b in buf.minibatches(64))
        buf.next_rollout()
        assert buf.mem_store is None and buf.memory is None
    finally:
        env.close()


# ---- prev flush against out ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [("out", "prev"), ("prev", "out")], ids=["prev_behind_out", "prev_before_out"])
@pytest.mark.parametrize("W,H,rows", [(15, 15, 67), (5, 6, 3)], ids=["15x15", "5x6"])          # 5x6: a row is no multiple of a wave or of 16 bytes
def test_prev_flush_against_out(W, H, rows, order):
    """prev = out + STATE bytes and prev = out - STATE pass the argument checks (test_memory_api.py): there a store one
    element past out's end, or one before its start, lands in the previous state.  obs, reset, prev and out are carved out of
    one device allocation (tests/_slab.py); one update from a random previous state with some rows reset: out is the
    reference's bit for bit, prev, obs and reset are what was uploaded, guard bands and gaps untouched."""
    from _slab import Slab
    rpf, cap = 1, 64
    obs, reset = _sequence(W, H, rows, rpf)
    ref = _reference(W, H, rows, rpf, cap)
    s = next(s for s in range(1, STEPS) if 0 < int(reset[s].sum()) < rows)                     # some rows reset, not all
    STATE = rows * 4 * H * W * 4
    slab = Slab({"obs": rows * 9 * H * W * 4, "reset": rows // rpf, "prev": STATE, "out": STATE}, (order, ("obs",), ("reset",)))
    assert slab.offsets[order[1]] - slab.offsets[order[0]] == STATE
    slab.put("obs", obs[s])
    slab.put("reset", reset[s])
    slab.put("prev", ref[s - 1])
    slab.upload(_torch(), _dev())
    hip_update(slab.at("obs"), slab.at("prev"), slab.at("reset"), slab.at("out"), W, H, cap, rows, rpf)   # raises unless 0
    assert not np.array_equal(ref[s].view(np.uint32), ref[s - 1].view(np.uint32))
    slab.check({"out": ref[s]}, f"{W}x{H}, {order}")
