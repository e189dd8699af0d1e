"""gvec_obs_symmetry and its front (symmetry.py) on the GPU against tests/_symmetry_reference.py: every result is compared
bit for bit (floats as their int32 views), so NaN payloads, -0.0 and denormals count."""
import ctypes as C
import functools

import numpy as np
import pytest

import _symmetry_reference as SR

pytestmark = pytest.mark.gpu

BOARDS = [(1, 1), (2, 2), (4, 4), (5, 3), (3, 5), (15, 15), (32, 32)]        # W x H
ROWS = [1, 5, 67]                                                             # 5: a partly filled last workgroup
SET_PLANES = (9, 9, 4, 5)                                                     # s, ns, memory, features


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _up(x):
    return _torch().from_numpy(np.array(x)).to(_dev())                        # a copy: the shared batches are read-only


def _bits(x):
    """a device float32 tensor as a host int32 array"""
    return x.detach().contiguous().view(_torch().int32).cpu().numpy()


def _same_bits(got, want):
    """the same float32 bits in the same order (leading dimensions may be grouped differently)"""
    return np.array_equal(_bits(got).reshape(-1), np.ascontiguousarray(want).view(np.int32).reshape(-1))


SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32)


def _float_bits(rng, shape):
    """float32 of random bit patterns: NaNs with payloads, both zeros, denormals and infinities among them"""
    bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1)
    at = rng.integers(0, flat.size, size=min(flat.size, 4 * SPECIALS.size))
    flat[at] = SPECIALS[np.arange(at.size) % SPECIALS.size]
    return bits.view(np.float32)


def _syms(rows, offset):
    """every symmetry in turn, so that a batch of eight rows or more holds all of them"""
    return ((np.arange(rows) + offset) % 8).astype(np.uint8)


@functools.lru_cache(maxsize=4)
def _batch(W, H, rows):
    """planes (one array per set), mask, values, action of a batch - drawn once, left unchanged"""
    rng = np.random.default_rng(10000 * W + 100 * H + rows)
    A = 5 * H * W
    planes = tuple(_float_bits(rng, (rows, p, H, W)) for p in SET_PLANES)
    mask = rng.random((rows, A)) < 0.4
    values = _float_bits(rng, (rows, A))
    action = rng.integers(0, A, size=rows)
    half = rng.random(rows) < 0.5                       # half of the rows play a half move
    action = np.where(half, 5 * (action // 5) + 4, action).astype(np.int64)
    if rows >= 8:
        action[1], action[2] = -1, A                    # out of range: copied, and no rule
    for x in planes + (mask, values, action):
        x.setflags(write=False)
    return planes, mask, values, action


# ---- every board, every row count: four plane sets, mask, values and action in one launch -------------------------------

@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("W,H", BOARDS)
def test_one_launch_against_the_reference(W, H, rows):
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry
    planes, mask, values, action = _batch(W, H, rows)
    d_planes = [_up(p) for p in planes]
    wide = t.full((2 * rows, 9, H, W), float("nan"), device=_dev())           # set 0 is read in place from every second row
    wide[::2] = d_planes[0]
    d_planes[0] = wide[::2]
    d_mask, d_values, d_action = _up(mask), _up(values), _up(action)
    for offset in range(0, 8, max(1, min(rows, 8))):                          # rows < 8: further calls until every sym was used
        sym = _syms(rows, offset)
        if rows >= 8:
            sym[3], sym[4] = 8, 255                                           # no symmetry: the identity, applied 0
        want_p, want_m, want_v, want_a, want_applied = SR.apply(sym, H, W, planes, mask, values, action)
        got = apply_symmetry(_up(sym), tuple(d_planes), mask=d_mask, values=d_values, action=d_action, return_applied=True)
        assert len(got) == 8
        for k in range(4):
            assert got[k].shape == (rows, SET_PLANES[k], H, W) and _same_bits(got[k], want_p[k]), (k, offset)
        assert got[4].dtype == t.bool and np.array_equal(got[4].cpu().numpy(), want_m), offset
        assert _same_bits(got[5], want_v), offset
        assert got[6].dtype == t.int64 and np.array_equal(got[6].cpu().numpy(), want_a), offset
        assert got[7].dtype == t.uint8 and np.array_equal(got[7].cpu().numpy(), want_applied), offset
        if W != H:                                                            # sym >= 4 does not exist there
            assert (want_applied[sym >= 4] == 0).all()
        if rows >= 8:
            assert want_applied[3] == 0 and want_applied[4] == 0 and want_a[1] == -1 and want_a[2] == 5 * H * W


@pytest.mark.parametrize("W,H", [(4, 4), (15, 15)])
@pytest.mark.parametrize("sym", range(8))
def test_each_symmetry_alone_and_each_tensor_alone(W, H, sym):
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry
    rows = 5
    planes, mask, values, action = _batch(W, H, rows)
    full = np.where(action % 5 == 4, action - 1, action)                      # full moves: the int sym holds for every row
    want_p, want_m, want_v, want_a, applied = SR.apply(np.full(rows, sym, np.uint8), H, W, planes[2:3], mask, values, full)
    assert (applied == sym).all()
    one = _up(planes[2][:, :1])                                               # a set of one plane
    kw = dict(height=H, width=W)
    (got,) = apply_symmetry(sym, one)
    assert got.shape == (rows, 1, H, W) and _same_bits(got, want_p[0][:, :1])
    (got,) = apply_symmetry(sym, mask=_up(mask), **kw)
    assert got.dtype == t.bool and np.array_equal(got.cpu().numpy(), want_m)
    (got,) = apply_symmetry(sym, mask=_up(mask.astype(np.uint8) * 3), **kw)   # uint8 bytes are moved, not normalised
    assert got.dtype == t.uint8 and np.array_equal(got.cpu().numpy(), want_m.astype(np.uint8) * 3)
    (got,) = apply_symmetry(sym, values=_up(values), **kw)
    assert _same_bits(got, want_v)
    got_m, got_v = apply_symmetry(sym, mask=_up(mask), values=_up(values), **kw)
    assert np.array_equal(got_m.cpu().numpy(), want_m) and _same_bits(got_v, want_v)
    got_a, got_applied = apply_symmetry(sym, action=_up(full), return_applied=True, **kw)
    assert np.array_equal(got_a.cpu().numpy(), want_a) and (got_applied.cpu().numpy() == sym).all()
    # leading shape (rows, 1) and a tensor sym
    got_p, got_a = apply_symmetry(t.full((rows, 1), sym, dtype=t.uint8, device=_dev()), _up(planes[2]).unsqueeze(1),
                                  action=_up(full).unsqueeze(1))
    assert got_p.shape == (rows, 1, 4, H, W) and _same_bits(got_p, want_p[0]) and np.array_equal(got_a.cpu().numpy()[:, 0], want_a)


def test_strided_view_equals_its_contiguous_copy_and_empty_batches():
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry
    W, H, rows = 15, 15, 67
    planes, _, _, _ = _batch(W, H, rows)
    wide = t.zeros((2 * rows, 9, H, W), device=_dev())
    wide[::2] = _up(planes[0])
    sym = _up(_syms(rows, 0))
    view = wide[::2]
    assert not view.is_contiguous()
    (a,), (b,) = apply_symmetry(sym, view), apply_symmetry(sym, view.contiguous())
    assert t.equal(a.view(t.int32), b.view(t.int32)) and _same_bits(a, SR.apply(_syms(rows, 0), H, W, planes[:1])[0][0])
    # planes that are not dense inside a row are copied first: the same result
    cut = _up(planes[0])[:, :, :, :7]
    (c,) = apply_symmetry(sym % 4, cut)
    assert _same_bits(c, SR.apply(_syms(rows, 0) % 4, H, 7, [np.ascontiguousarray(planes[0][:, :, :, :7])])[0][0])
    empty = apply_symmetry(sym[:0], wide[:0], action=t.zeros(0, dtype=t.int64, device=_dev()), return_applied=True)
    assert [tuple(x.shape) for x in empty] == [(0, 9, H, W), (0,), (0,)]


# ---- large launches: transposed rows go through LDS ----------------------------------------------------------------------
# launch_obs_symmetry stages them when the board is square, 13 wide or more, and the launch has 4,096 rows or more: the row
# counts on either side of that, the smallest such board, the widest (the most LDS; fewer planes, to keep the case small), an
# even and an odd width, and a board just too small.
STAGED = [(13, 4095), (13, 4096), (12, 4096), (15, 4096), (20, 4097), (32, 4096)]


@pytest.mark.parametrize("n,rows", STAGED)
def test_large_launches_against_the_reference(n, rows):
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry
    W = H = n
    A = 5 * H * W
    rng = np.random.default_rng(n * 100000 + rows)
    bits = lambda *shape: rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)      # noqa: E731
    # passes of three planes through LDS: three full ones, a full and a partial one, partial ones alone
    planes = [bits(rows, p, H, W) for p in ((9, 4, 1, 2) if n < 32 else (4, 1, 2, 1))]
    mask, values = rng.random((rows, A)) < 0.4, bits(rows, A)
    action = rng.integers(0, A, size=rows).astype(np.int64)
    action[:64] = np.arange(64) % A // 5 * 5 + 4                              # half moves too: rows that fall back among staged ones
    sym = _syms(rows, 0)
    sym[-1] = 4                                                               # the last row of the launch transposed
    want_p, want_m, want_v, want_a, want_applied = SR.apply(sym, H, W, planes, mask, values, action)
    got = apply_symmetry(_up(sym), tuple(_up(p) for p in planes), mask=_up(mask), values=_up(values), action=_up(action),
                         return_applied=True)
    for k in range(4):
        assert _same_bits(got[k], want_p[k]), k
    assert np.array_equal(got[4].cpu().numpy(), want_m) and _same_bits(got[5], want_v)
    assert np.array_equal(got[6].cpu().numpy(), want_a) and np.array_equal(got[7].cpu().numpy(), want_applied)
    # the mask alone, at every alignment of its rows, and inverse
    (m_only,) = apply_symmetry(_up(sym), mask=_up(mask), height=H, width=W)
    assert np.array_equal(m_only.cpu().numpy(), SR.apply(sym, H, W, mask=mask)[1])
    (back,) = apply_symmetry(_up(sym), got[0], action=_up(action), inverse=True)[:1]
    assert _same_bits(back, planes[0])


# ---- actions: every tile and direction, and the half-move rule -------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(4, 4), (5, 3)])
def test_every_action_under_every_symmetry(W, H):
    from generalsreinforcementlearning_amd import apply_symmetry
    A, n = 5 * H * W, SR.num_symmetries(H, W)
    per = np.concatenate([np.arange(A), [-1, A]]).astype(np.int64)            # 80 (75) actions, and two out of range
    action = np.tile(per, n)
    sym = np.repeat(np.arange(n), per.size).astype(np.uint8)
    rows = action.size
    rng = np.random.default_rng(W * 10 + H)
    planes = [_float_bits(rng, (rows, 9, H, W))]
    mask, values = rng.random((rows, A)) < 0.4, _float_bits(rng, (rows, A))
    want_p, want_m, want_v, want_a, want_applied = SR.apply(sym, H, W, planes, mask, values, action)
    got_p, got_m, got_v, got_a, got_applied = apply_symmetry(_up(sym), _up(planes[0]), mask=_up(mask), values=_up(values),
                                                             action=_up(action), return_applied=True)
    applied = got_applied.cpu().numpy()
    assert np.array_equal(applied, want_applied) and np.array_equal(got_a.cpu().numpy(), want_a)
    assert _same_bits(got_p, want_p[0]) and np.array_equal(got_m.cpu().numpy(), want_m) and _same_bits(got_v, want_v)
    inside = (action >= 0) & (action < A)
    half = inside & (action % 5 == 4)
    assert (applied[~half] == sym[~half]).all()                               # full moves and out-of-range actions restrict nothing
    assert np.array_equal(got_a.cpu().numpy()[~inside], action[~inside])
    fell = half & (applied != sym)
    assert (applied[fell] == 0).all()
    if (W, H) == (4, 4):
        for s in range(8):
            kept, back = int((half & (sym == s) & (applied == s)).sum()), int((fell & (sym == s)).sum())
            assert (kept, back) == ([16, 12, 2, 2, 0, 4, 4, 6][s], 16 - [16, 12, 2, 2, 0, 4, 4, 6][s])
            if s not in (0, 4):
                assert kept > 0 and back > 0
    # a half move that falls back comes out as it went in, in every tensor
    assert fell.any()
    assert np.array_equal(_bits(got_p)[fell], planes[0].view(np.int32)[fell])
    assert np.array_equal(got_m.cpu().numpy()[fell], mask[fell]) and np.array_equal(_bits(got_v)[fell], values.view(np.int32)[fell])
    assert np.array_equal(got_a.cpu().numpy()[fell], action[fell])


@pytest.mark.parametrize("W,H", [(4, 4), (5, 3), (15, 15)])
def test_inverse_restores_every_input(W, H):
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry, inverse_symmetry
    rows = 67
    planes, mask, values, action = _batch(W, H, rows)
    sym = _up(_syms(rows, 3) % SR.num_symmetries(H, W))
    d_in = [_up(planes[0]), _up(planes[2])]
    d_mask, d_values, d_action = _up(mask), _up(values), _up(action)
    p0, p1, m, v, a, applied = apply_symmetry(sym, tuple(d_in), mask=d_mask, values=d_values, action=d_action, return_applied=True)
    fell = (applied != sym).cpu().numpy()
    assert fell.any() and not fell.all()
    q0, q1, qm, qv, _, again = apply_symmetry(sym, (p0, p1), mask=m, values=v, action=d_action, inverse=True, return_applied=True)
    assert t.equal(again, applied)
    assert t.equal(q0.view(t.int32), d_in[0].view(t.int32)) and t.equal(q1.view(t.int32), d_in[1].view(t.int32))
    assert t.equal(qm, d_mask) and t.equal(qv.view(t.int32), d_values.view(t.int32))
    # the action goes back through a forward call with the inverse of what was applied
    back, applied_back = apply_symmetry(inverse_symmetry(applied), action=a, height=H, width=W, return_applied=True)
    assert t.equal(back, d_action) and t.equal(applied_back, inverse_symmetry(applied))
    want = SR.apply(sym.cpu().numpy(), H, W, [_bits(p0).view(np.float32)], action=action, inverse=True)
    assert np.array_equal(want[0][0].view(np.int32), planes[0].view(np.int32))            # the reference agrees on what inverse means


# ---- against the kernels the symmetries must commute with ---------------------------------------------------------------

def _random_legal(t, mask, gen):
    """one legal action per row of a bool mask [..., A] (0 where a row has none)"""
    m = mask.reshape(-1, mask.shape[-1]).float()
    m[m.sum(1) == 0, 0] = 1.0
    return t.multinomial(m, 1, generator=gen).squeeze(1).reshape(mask.shape[:-1])


def test_mask_and_features_commute_on_a_real_env():
    t = _torch()
    from generalsreinforcementlearning_amd import apply_symmetry, strategic_features, valid_actions_mask_from_observation
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    B, W, H = 64, 8, 8
    env = GeneralsVecEnv(B, W, H, max_turns=100, device_outputs=True, seed=3)
    gen = t.Generator(device=_dev())
    gen.manual_seed(11)
    try:
        obs, info = env.reset()
        for _ in range(30):
            obs, _, _, _, info = env.step(_random_legal(t, info["valid_actions_mask"].bool(), gen))
        obs, mask = obs.clone(), info["valid_actions_mask"].bool().clone()
    finally:
        env.close()
    assert int(mask.sum()) > B                                                # boards 30 turns in: more than one legal move each
    feats = strategic_features(obs)
    for k in range(8):
        t_obs, t_feats, t_mask = apply_symmetry(k, (obs, feats), mask=mask)
        assert t.equal(valid_actions_mask_from_observation(t_obs), t_mask), k
        assert t.equal(strategic_features(t_obs).view(t.int32), t_feats.view(t.int32)), k
    # ... and with a symmetry of its own per row
    sym = _up(_syms(B, 0))
    t_obs, t_feats, t_mask = apply_symmetry(sym, (obs, feats), mask=mask)
    assert t.equal(valid_actions_mask_from_observation(t_obs), t_mask)
    assert t.equal(strategic_features(t_obs).view(t.int32), t_feats.view(t.int32))


def test_memory_planes_commute_on_a_self_play_env():
    t = _torch()
    from generalsreinforcementlearning_amd import (ObservationMemory, apply_symmetry, strategic_features,
                                                   valid_actions_mask_from_observation)
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, W, H, L = 64, 9, 7, 2
    env = GeneralsSelfPlayVecEnv(B, W, H, max_players=2, max_turns=12, device_outputs=True, seed=9)
    gen = t.Generator(device=_dev())
    gen.manual_seed(5)
    sym = _up((_syms(B * L, 0) % 4).reshape(B, L))                            # not square: four symmetries, one per learner's view
    plain, moved = ObservationMemory((B, L), H, W), ObservationMemory((B, L), H, W)
    try:
        obs, info = env.reset()
        flags = None
        for step in range(31):
            mem = plain.update(obs, flags)
            mask = info["valid_actions_mask"].bool()
            t_obs, t_mem, t_mask = apply_symmetry(sym, (obs, mem), mask=mask)
            assert t.equal(moved.update(t_obs, flags).view(t.int32), t_mem.view(t.int32)), step
            assert t.equal(valid_actions_mask_from_observation(t_obs), t_mask), step
            assert t.equal(strategic_features(t_obs).view(t.int32), apply_symmetry(sym, strategic_features(obs))[0].view(t.int32)), step
            obs, _, _, _, info = env.step(_random_legal(t, mask, gen))
            flags = info["reset"]
        assert bool((mem[..., 0, :, :] == 1.0).any()) and bool((mem[..., 0, :, :] == 0.0).any())   # seen and never seen tiles
    finally:
        env.close()


# ---- nothing but the outputs is written ------------------------------------------------------------------------------------

def _raw(sym, W, H, sets, mask=None, values=None, action=None, applied=None, inverse=0):
    """the C entry point on device tensors whose data_ptr() is row 0: sets of (in, out, planes, in_row_stride)"""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import ObsSymmetryArgs, check
    a = ObsSymmetryArgs(rows=sym.numel(), width=W, height=H, num_sets=len(sets), inverse=inverse, reserved=0, sym=sym.data_ptr())
    for k, (src, dst, planes, stride) in enumerate(sets):
        a.sets[k].in_, a.sets[k].out, a.sets[k].planes, a.sets[k].in_row_stride = src.data_ptr(), dst.data_ptr(), planes, stride
    if mask:
        a.mask_in, a.mask_out = mask[0].data_ptr(), mask[1].data_ptr()
    if values:
        a.values_in, a.values_out = values[0].data_ptr(), values[1].data_ptr()
    if action:
        a.action_in, a.action_out = action[0].data_ptr(), action[1].data_ptr()
    if applied is not None:
        a.applied = applied.data_ptr()
    check(g.load().gvec_obs_symmetry(0, _torch().cuda.current_stream(_dev()).cuda_stream, C.byref(a)), "gvec_obs_symmetry")


@pytest.mark.parametrize("W,H,rows", [(15, 15, 5), (3, 5, 67), (32, 32, 5), (15, 15, 4099)])                     # the last: staged through LDS
def test_guard_bands_and_a_second_call(W, H, rows):
    """every output sits between guard bands at an odd byte offset of its buffer (mask rows then start at every alignment),
    and a second call into other buffers leaves the first call's outputs alone"""
    t = _torch()
    planes, mask, values, action = _batch(W, H, rows)
    A, G = 5 * H * W, 64                                                      # G elements of guard on either side
    sym = _syms(rows, 1) % SR.num_symmetries(H, W)
    want_p, want_m, want_v, want_a, want_applied = SR.apply(sym, H, W, planes, mask, values, action)

    def guarded(numel, dtype, fill, shift=0):
        buf = t.full((numel + 2 * G + shift,), fill, dtype=dtype, device=_dev())
        return buf, buf[G + shift:G + shift + numel]

    def launch(shift):
        outs = [guarded(rows * p * H * W, t.int32, -7) for p in SET_PLANES]
        o_mask, o_values = guarded(rows * A, t.uint8, 0xAB, shift), guarded(rows * A, t.int32, -7)
        o_action, o_applied = guarded(rows, t.int64, -7), guarded(rows, t.uint8, 0xAB, shift)
        ins = [_up(p) for p in planes]
        _raw(_up(sym), W, H, [(ins[k], outs[k][1], SET_PLANES[k], SET_PLANES[k] * H * W) for k in range(4)],
             mask=(_up(mask), o_mask[1]), values=(_up(values), o_values[1]), action=(_up(action), o_action[1]), applied=o_applied[1])
        return outs, o_mask, o_values, o_action, o_applied

    def check_all(res, shift):
        outs, o_mask, o_values, o_action, o_applied = res
        for k in range(4):
            buf, view = outs[k]
            assert np.array_equal(view.cpu().numpy(), want_p[k].view(np.int32).reshape(-1)), k
            assert bool((buf[:G] == -7).all()) and bool((buf[-G:] == -7).all()), k
        for (buf, view), want, fill in ((o_mask, want_m.astype(np.uint8).reshape(-1), 0xAB), (o_values, want_v.view(np.int32).reshape(-1), -7),
                                        (o_action, want_a, -7), (o_applied, want_applied, 0xAB)):
            assert np.array_equal(view.cpu().numpy(), want)
            assert bool((buf[:view.storage_offset()] == fill).all()) and bool((buf[view.storage_offset() + view.numel():] == fill).all())

    first = launch(1)
    t.cuda.synchronize()
    snapshot = [x[1].clone() for x in first[0]] + [first[1][1].clone(), first[2][1].clone()]
    others = [launch(shift) for shift in (0, 2, 3)]                            # further calls, on the same stream, into other buffers
    t.cuda.synchronize()
    check_all(first, 1)
    for res, shift in zip(others, (0, 2, 3)):
        check_all(res, shift)
    for before, after in zip(snapshot, [x[1] for x in first[0]] + [first[1][1], first[2][1]]):
        assert t.equal(before, after)


# ---- buffers that exactly touch ---------------------------------------------------------------------------------------------
# The entry point accepts an output whose first byte is the first byte behind an input, and one whose last byte is the last
# before it.  There a store one element past an end - a mask head or tail at the wrong alignment, the last slot of a strided
# row - lands in live input data, not in a guard band or the allocator's slack.  Every buffer of these launches is carved out
# of one device allocation (tests/_slab.py), so the distances are exact; after the launch every output is the reference's bit
# for bit, every input what was uploaded, and the guard bands and gaps untouched.
TOUCH_W = TOUCH_H = 15
TOUCH_BUFFERS = ("sym", "in", "out", "mask_in", "mask_out", "values_in", "values_out", "action_in", "action_out", "applied")


@functools.lru_cache(maxsize=None)
def _touching_batch(rows, planes):
    """(inputs, the reference's outputs) of a 15x15 launch of one plane set with mask, values, action and applied - drawn
    once, left unchanged.  From nine rows on every symmetry and the out-of-range 8 occur in turn (three rows: 4, 5, 6); a few
    rows play a half move from the middle of the board, which sym 1 keeps and sym 2 turns into the identity."""
    W, H = TOUCH_W, TOUCH_H
    A = 5 * H * W
    rng = np.random.default_rng(77000 + 10 * rows + planes)
    sym = ((np.arange(rows) + (4 if rows < 8 else 0)) % 9).astype(np.uint8)
    p = _float_bits(rng, (rows, planes, H, W))
    mask = rng.integers(0, 256, size=(rows, A), dtype=np.uint8)              # any byte: they are moved, not normalised
    values = _float_bits(rng, (rows, A))
    action = (5 * rng.integers(0, H * W, size=rows) + rng.integers(0, 4, size=rows)).astype(np.int64)
    action[np.isin(np.arange(rows) % 64, (1, 2, 5))] = 5 * (7 * W + 7) + 4
    if rows > 16:
        action[9], action[10] = -1, A
    want_p, want_m, want_v, want_a, applied = SR.apply(sym, H, W, [p], mask, values, action)
    if rows >= 9:
        assert set(sym[:9]) == set(range(9)) and applied[8] == 0
        assert applied[1] == 1 and sym[2] == 2 and applied[2] == 0           # applied differs from sym, and not in every half move
    ins = dict(sym=sym, planes=p, mask_in=mask, values_in=values, action_in=action)
    outs = dict(out=want_p[0], mask_out=want_m, values_out=want_v, action_out=want_a, applied=applied)
    for x in list(ins.values()) + list(outs.values()):
        x.setflags(write=False)
    return ins, outs


def _launch_touching(rows, groups, distances, planes=9, stride=None, shift=None, mask_out_alignment=None):
    """one launch of _touching_batch(rows, planes): the buffers of each group flush against each other in the order given, the
    others apart.  distances: (a, b, bytes) with b's first byte that many behind a's, as the entry point's range check counts."""
    from _slab import FILL, Slab
    W, H = TOUCH_W, TOUCH_H
    HW, A = H * W, 5 * H * W
    row = planes * HW
    stride = row if stride is None else stride
    in_floats = (rows - 1) * stride + row                                     # as far as a strided input reaches
    ins, outs = _touching_batch(rows, planes)
    sizes = {"sym": rows, "applied": rows, "in": in_floats * 4, "out": rows * row * 4, "mask_in": rows * A, "mask_out": rows * A,
             "values_in": rows * A * 4, "values_out": rows * A * 4, "action_in": rows * 8, "action_out": rows * 8}
    flush = {name for g in groups for name in g}
    slab = Slab(sizes, tuple(groups) + tuple((name,) for name in TOUCH_BUFFERS if name not in flush), shift)
    for a, b, nbytes in distances:
        assert slab.offsets[b] - slab.offsets[a] == nbytes, (a, b)
    spread = np.full(in_floats, FILL * 0x01010101, np.uint32)                 # the rows of the input, stride apart
    for r in range(rows):
        spread[r * stride:r * stride + row] = ins["planes"][r].view(np.uint32).reshape(-1)
    slab.put("in", spread)
    for name in ("sym", "mask_in", "values_in", "action_in"):
        slab.put(name, ins[name])
    slab.upload(_torch(), _dev())
    at = slab.at
    if mask_out_alignment is not None:
        assert at("mask_out").data_ptr() % 4 == mask_out_alignment
    _raw(at("sym"), W, H, [(at("in"), at("out"), planes, stride)], mask=(at("mask_in"), at("mask_out")),
         values=(at("values_in"), at("values_out")), action=(at("action_in"), at("action_out")), applied=at("applied"))   # raises unless 0
    slab.check(outs, f"{rows} rows, {groups}")


def _seams(rows, planes=9):
    """name -> arguments of _launch_touching: which buffers touch, and the byte distance that says so"""
    HW, A = TOUCH_H * TOUCH_W, 5 * TOUCH_H * TOUCH_W
    state = rows * planes * HW * 4
    strided = ((rows - 1) * 2 * planes * HW + planes * HW) * 4                # the first byte behind the last row's payload
    seams = {"out_behind_in": dict(groups=[("in", "out")], distances=[("in", "out", state)]),
             "out_before_in": dict(groups=[("out", "in")], distances=[("out", "in", state)]),
             "out_behind_strided_in": dict(groups=[("in", "out")], distances=[("in", "out", strided)], stride=2 * planes * HW),
             "applied_behind_sym": dict(groups=[("sym", "applied")], distances=[("sym", "applied", rows)]),
             "applied_before_sym": dict(groups=[("applied", "sym")], distances=[("applied", "sym", rows)]),
             "values_out_behind_values_in": dict(groups=[("values_in", "values_out")], distances=[("values_in", "values_out", rows * A * 4)]),
             "mask_in_behind_mask_out": dict(groups=[("mask_out", "mask_in")], distances=[("mask_out", "mask_in", rows * A)],
                                             shift={"mask_out": 3}, mask_out_alignment=3)}
    for k in range(4):                                                        # the seam at each byte alignment: head and tail stores
        seams[f"mask_out_behind_mask_in_at_{k}"] = dict(groups=[("mask_in", "mask_out")], distances=[("mask_in", "mask_out", rows * A)],
                                                        shift={"mask_in": (k - rows * A) % 4}, mask_out_alignment=k)
    return seams


@pytest.mark.parametrize("seam", sorted(_seams(9)))
def test_an_output_flush_against_an_input(seam):
    _launch_touching(9, **_seams(9)[seam])


# the argument sets that test_symmetry_api.py pins as accepted (3 rows: out = in + 24,300 bytes, in - 24,300, a strided in's
# end, applied = sym + 3) are launched there only where no device is; here they return 0 on real memory and compute the reference
@pytest.mark.parametrize("seam", ["out_behind_in", "out_before_in", "out_behind_strided_in", "applied_behind_sym"])
def test_the_accepted_touching_arguments_of_the_api_test(seam):
    case = _seams(3)[seam]
    assert case["distances"][0][2] == {"out_behind_in": 24300, "out_before_in": 24300, "out_behind_strided_in": (2 * 4050 + 2025) * 4,
                                       "applied_behind_sym": 3}[seam]
    _launch_touching(3, **case)


def test_a_staged_launch_with_outputs_flush_against_inputs():
    """4,096 rows of 15x15, the smallest launch whose transposed rows go through LDS, with four planes (a full pass of three and
    a partial one): out directly behind in, mask_out directly behind mask_in"""
    rows, planes = 4096, 4
    ins, _ = _touching_batch(rows, planes)
    assert (ins["sym"] & 4).any() and rows >= 4096 and TOUCH_W >= 13
    _launch_touching(rows, [("in", "out"), ("mask_in", "mask_out")], planes=planes,
                     distances=[("in", "out", rows * planes * 225 * 4), ("mask_in", "mask_out", rows * 1125)])
