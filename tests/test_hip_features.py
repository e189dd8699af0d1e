"""The strategic feature planes on the GPU (gvec_obs_features, features.strategic_features, the envs' option) against the
numpy restatement of tests/_features_reference.py.

cap is a power of two, so min(d, cap) / cap is an exact float32 whatever computes it: every comparison is np.array_equal.
There is no tolerance.  The reference's breadth-first search runs once per board shape (distances_one, uncapped); the caps
and the row counts of the cases share it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _features_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(5, 5), (8, 8), (15, 15), (20, 20), (32, 32), (32, 3), (3, 32)]     # W x H
ROWS = [1, 3, 67]
CAPS = [2, 64, 1024]


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def hip_features(obs, W, H, cap, stride=None, out=None, rows=None):
    """the C entry point on device tensors: obs any float32 tensor whose data_ptr() is observation 0"""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import ObsFeaturesArgs, check
    t = _torch()
    rows = obs.shape[0] if rows is None else rows
    if out is None:
        out = t.full((rows, 5, H, W), np.nan, dtype=t.float32, device=_dev())
    a = ObsFeaturesArgs(rows=rows, width=W, height=H, cap=cap, reserved=0, obs_row_stride=9 * W * H if stride is None else stride,
                        obs=obs.data_ptr(), out=out.data_ptr())
    check(g.load().gvec_obs_features(0, t.cuda.current_stream(_dev()).cuda_stream, C.byref(a)), "gvec_obs_features")
    return out


@functools.lru_cache(maxsize=None)
def _random_case(W, H, mountain_share):
    """(observations [67, 9, H, W], their uncapped reference distances and front lines) - computed once, left unchanged"""
    rng = np.random.default_rng(1000 * W + 10 * H + int(100 * mountain_share))
    obs = R.random_obs(rng, max(ROWS), H, W, mountain_share=mountain_share)
    ref = [R.distances_one(o) for o in obs]
    obs.setflags(write=False)
    return obs, ref


def _expected(ref, rows, cap):
    return np.stack([R.apply_cap(d, f, cap) for d, f in ref[:rows]])


@pytest.mark.parametrize("mountain_share", [0.2, 0.45])
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_bit_exact_against_the_reference(W, H, mountain_share):
    t = _torch()
    obs, ref = _random_case(W, H, mountain_share)
    d_obs = t.from_numpy(obs.copy()).to(_dev())
    for rows in ROWS:
        for cap in CAPS:
            want = _expected(ref, rows, cap)
            got = hip_features(d_obs[:rows].contiguous(), W, H, cap).cpu().numpy()
            assert not np.isnan(got).any(), "an element was not written"
            share = float((want[:, :4] < 1.0).mean())
            print(f"{W}x{H} mountains {mountain_share} rows {rows} cap {cap}: {share:.3f} of the distance values < 1.0, "
                  f"deepest level {max(int(d.max()) for d, _ in ref[:rows])}")
            if mountain_share == 0.2:
                # Not vacuous: at least 40 % of these rows' plane 0-3 values are below 1.0 (64-88 % here at cap 64 and 1024).
                # cap = 2 leaves only d <= 1 below 1.0 whatever the board (26-36 % here), so there the same rows are held to
                # the bound at the default cap: it is the inputs that must not be empty.
                assert float((_expected(ref, rows, max(cap, 64))[:, :4] < 1.0).mean()) >= 0.40, share
            assert np.array_equal(got, want), (rows, cap, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("n,cap,depth", [(9, 32, 48), (32, 1024, 527), (31, 64, 510)])
def test_serpentine(n, cap, depth):
    t = _torch()
    obs = R.serpentine(n)
    assert R.max_depth(obs) == depth
    got = hip_features(t.from_numpy(obs[None]).to(_dev()), n, n, cap).cpu().numpy()[0]
    want = R.features_one(obs, cap)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if n == 9:
        assert int((got[0][obs[4] == 0] == 1.0).sum()) == 17


def test_hand_written_boards():
    """the boards tests/test_features_reference.py pins the reference on, through the kernel"""
    t = _torch()
    b = lambda rows: np.array([[c == "#" for c in r] for r in rows], bool)
    boards = [
        (R.make_obs(3, 3, mtn=b(["...", ".#.", "..."]), gen=b(["#..", "...", "..."]), mine=b(["#..", "..#", "..."]), enemy=b(["...", "...", "..#"])), 8),
        (R.make_obs(1, 5, enemy=b(["....#"]), vis=b([".####"])), 4),
        (R.make_obs(2, 4, enemy=b(["...#", "...."])), 8),
        (R.make_obs(2, 4, enemy=b(["....", "#..."])), 8),
        (R.make_obs(4, 3, mtn=b(["#..", "...", "...", "..#"])), 64),
        (R.make_obs(3, 3, mtn=b([".#.", "#.#", ".#."]), enemy=b(["...", ".#.", "..."])), 64),
        (R.make_obs(1, 3, mtn=b(["#.."]), enemy=b(["#.."])), 4),
        (R.make_obs(1, 1, enemy=b(["#"])), 2),
        (R.make_obs(32, 1, enemy=b(["#"] + ["."] * 31)), 16),
        (R.make_obs(1, 32, enemy=b(["." * 31 + "#"])), 32),
    ]
    for obs, cap in boards:
        H, W = obs.shape[1:]
        got = hip_features(t.from_numpy(obs[None]).to(_dev()), W, H, cap).cpu().numpy()[0]
        assert np.array_equal(got, R.features_one(obs, cap)), (H, W, cap, got)
    wrap = hip_features(t.from_numpy(boards[2][0][None]).to(_dev()), 4, 2, 8).cpu().numpy()[0]
    assert wrap[1, 1, 0] == np.float32(4 / 8)                            # the tile after column W - 1 is W steps away, not 1


def test_row_stride_and_untouched_gaps():
    t = _torch()
    W, H, rows, gap = 15, 15, 9, 13
    obs, ref = _random_case(W, H, 0.2)
    n = 9 * W * H
    big = t.full((rows, n + gap), 7.25, dtype=t.float32, device=_dev())
    big[:, :n] = t.from_numpy(obs[:rows].reshape(rows, n).copy()).to(_dev())
    before = big.clone()
    got = hip_features(big, W, H, 64, stride=n + gap, rows=rows).cpu().numpy()
    assert np.array_equal(got, _expected(ref, rows, 64))
    assert t.equal(big, before)                                          # the floats between rows (and the rows) are untouched
    # the Python front reads the same view in place
    from generalsreinforcementlearning_amd import strategic_features
    view = big[:, :n].view(rows, 9, H, W)
    assert not view.is_contiguous()
    assert np.array_equal(strategic_features(view).cpu().numpy(), got)


@pytest.mark.parametrize("W,H", [(15, 15), (20, 20), (5, 5)], ids=["15x15", "20x20", "5x5"])
def test_base_pointers_off_16_byte_alignment(W, H):
    t = _torch()
    rows = 5
    obs, ref = _random_case(W, H, 0.2)
    want = _expected(ref, rows, 64)
    n_in, n_out = rows * 9 * W * H, rows * 5 * W * H
    for off_in in range(4):
        for off_out in range(4):
            src = t.zeros(n_in + 8, dtype=t.float32, device=_dev())
            src[off_in:off_in + n_in] = t.from_numpy(obs[:rows].reshape(-1).copy()).to(_dev())
            dst = t.full((n_out + 4 + 16,), -3.5, dtype=t.float32, device=_dev())
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            hip_features(src[off_in:], W, H, 64, out=dst[off_out:], rows=rows)
            d = dst.cpu().numpy()
            assert np.array_equal(d[off_out:off_out + n_out].reshape(rows, 5, H, W), want), (off_in, off_out)
            assert (d[:off_out] == -3.5).all() and (d[off_out + n_out:] == -3.5).all(), (off_in, off_out)   # the sentinel after out's end


def test_unread_planes_and_the_all_zero_observation():
    t = _torch()
    W, H, rows = 20, 20, 4
    obs, _ = _random_case(W, H, 0.2)
    a = obs[:rows].copy()
    b = a.copy()
    rng = np.random.default_rng(3)
    for p in (2, 3, 7, 8):
        b[:, p] = rng.random((rows, H, W), dtype=np.float32) * 9 - 4
    fa = hip_features(t.from_numpy(a).to(_dev()), W, H, 64).cpu().numpy()
    fb = hip_features(t.from_numpy(b).to(_dev()), W, H, 64).cpu().numpy()
    assert np.array_equal(fa, fb)
    zero = hip_features(t.zeros((2, 9, H, W), dtype=t.float32, device=_dev()), W, H, 64).cpu().numpy()
    assert (zero[:, 3] == 0.0).all() and (zero[:, :3] == 1.0).all() and (zero[:, 4] == 0.0).all()
    assert np.array_equal(zero[0], R.features_one(np.zeros((9, H, W), np.float32), 64))


def test_python_front_shapes_and_outputs():
    t = _torch()
    from generalsreinforcementlearning_amd import strategic_features
    W, H = 8, 8
    obs, ref = _random_case(W, H, 0.2)
    want = _expected(ref, 6, 16)
    x = t.from_numpy(obs[:6].copy()).to(_dev()).requires_grad_(True)
    f = strategic_features(x.view(3, 2, 9, H, W), cap=16)
    assert f.shape == (3, 2, 5, H, W) and not f.requires_grad and f.grad_fn is None
    assert np.array_equal(f.cpu().numpy().reshape(6, 5, H, W), want)
    flat = strategic_features(x.detach().view(6, 9, H * W), cap=16, width=W, height=H)
    assert flat.shape == (6, 5, H * W) and np.array_equal(flat.cpu().numpy().reshape(6, 5, H, W), want)
    one = strategic_features(x.detach()[0], cap=16)
    assert one.shape == (5, H, W) and np.array_equal(one.cpu().numpy(), want[0])
    out = t.empty(6 * 5 * H * W, dtype=t.float32, device=_dev())
    r = strategic_features(x.detach(), cap=16, out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().reshape(6, 5, H, W), want)
    assert strategic_features(x.detach()[:0]).shape == (0, 5, H, W)
    odd = x.detach()[::2]                                                # no common stride with the planes: copied, same result
    assert np.array_equal(strategic_features(odd, cap=16).cpu().numpy(), want[::2])
    with pytest.raises(ValueError):
        strategic_features(x.detach(), out=t.empty(5, dtype=t.float32, device=_dev()))


FORMS = [(1, 1), (5, 6), (32, 32)]                                       # W x H


@pytest.mark.parametrize("W,H", FORMS, ids=[f"{w}x{h}" for w, h in FORMS])
def test_python_front_reads_every_form_of_a_batch(W, H):
    """six observations, handed over in every form the front accepts: the reference's planes whichever way they reach the kernel"""
    t = _torch()
    from generalsreinforcementlearning_amd import strategic_features
    from generalsreinforcementlearning_amd._obs_batch import in_place
    obs, ref = _random_case(W, H, 0.2)
    want, n, nan = _expected(ref, 6, 16), 9 * W * H, float("nan")
    x = t.from_numpy(obs[:6].copy()).to(_dev())
    got = lambda o, **k: strategic_features(o, cap=16, **k).cpu().numpy()
    assert np.array_equal(got(x.view(2, 3, 9, H, W)), want.reshape(2, 3, 5, H, W))          # leading shape (2, 3)
    assert np.array_equal(got(x.view(2, 3, 9, H * W), width=W, height=H), want.reshape(2, 3, 5, H * W))
    assert np.array_equal(got(x[0]), want[0])                                              # no leading shape
    assert np.array_equal(got(x[0].view(9, H * W), width=W, height=H), want[0].reshape(5, H * W))
    # rows of a wider tensor, NaN between them: read where they are
    wide = t.full((6, n + 13), nan, dtype=t.float32, device=_dev())
    wide[:, :n] = x.view(6, n)
    for view, tail in ((wide[:, :n].view(6, 9, H, W), 3), (wide[:, :n].view(6, 9, H * W), 2)):
        read, stride = in_place(view, tail, H, W)
        assert not view.is_contiguous() and read.data_ptr() == view.data_ptr() and stride == n + 13
        kw = dict(width=W, height=H) if tail == 2 else {}
        assert np.array_equal(got(view, **kw).reshape(6, 5, H, W), want)
    assert bool(wide[:, n:].isnan().all())
    # three of every four rows: no common stride, copied
    gappy = t.full((2, 4, 9, H, W), nan, dtype=t.float32, device=_dev())
    gappy[:, :3] = x.view(2, 3, 9, H, W)
    assert in_place(gappy[:, :3], 3, H, W)[0].data_ptr() != gappy.data_ptr()
    assert np.array_equal(got(gappy[:, :3]), want.reshape(2, 3, 5, H, W))
    # one observation expanded to six rows: stride 0, copied
    assert np.array_equal(got(x[:1].expand(6, 9, H, W)), np.repeat(want[:1], 6, axis=0))
    out = t.full((6 * 5 * H * W,), nan, dtype=t.float32, device=_dev())
    r = strategic_features(x.view(2, 3, 9, H, W), cap=16, out=out)
    assert r.data_ptr() == out.data_ptr() and r.shape == (2, 3, 5, H, W) and np.array_equal(out.cpu().numpy().reshape(6, 5, H, W), want)
    assert strategic_features(x[:0]).shape == (0, 5, H, W)
    assert strategic_features(x[:0].view(0, 3, 9, H * W), width=W, height=H, out=out[:0]).shape == (0, 3, 5, H * W)


# ---- the envs' option ----------------------------------------------------------------------------------------------

def _random_legal(t, mask, gen):
    """one legal action per row of a bool mask [..., A] (0 where a row has none)"""
    m = mask.reshape(-1, mask.shape[-1]).float()
    dead = m.sum(1) == 0
    m[dead, 0] = 1.0
    a = t.multinomial(m, 1, generator=gen).squeeze(1)
    return a.reshape(mask.shape[:-1])


def _check_info(obs, info, cap=64):
    got = info["strategic_features"]
    assert got.shape == obs.shape[:-3] + (5,) + obs.shape[-2:]
    assert np.array_equal(got.cpu().numpy(), R.features_batch(obs.cpu().numpy(), cap))


@pytest.mark.parametrize("kind", ["selfplay", "single"])
def test_env_info_carries_the_features(kind):
    t = _torch()
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    cls = GeneralsSelfPlayVecEnv if kind == "selfplay" else GeneralsVecEnv
    env = cls(64, 15, 15, max_players=4, device_outputs=True, strategic_features=True, seed=11)
    gen = t.Generator(device=_dev())
    gen.manual_seed(5)
    try:
        obs, info = env.reset()
        _check_info(obs, info)
        saved = None
        for step in range(30):
            obs, _, _, _, info = env.step(_random_legal(t, info["valid_actions_mask"], gen))
            _check_info(obs, info)
            if step == 14:
                saved = env.save_state()
        assert float((info["strategic_features"][..., :4, :, :] < 1.0).float().mean()) > 0.2
        obs, info = env.copy_envs(list(range(32, 64)), list(range(32)))
        _check_info(obs, info)
        obs, info = env.restore_state(saved)
        _check_info(obs, info)
        obs, _, _, _, info = env.step(_random_legal(t, info["valid_actions_mask"], gen))
        _check_info(obs, info)
    finally:
        env.close()


def test_env_option_off_leaves_info_as_it_was():
    t = _torch()
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    # the keys the envs hand out today, read from vector_env.py / selfplay_env.py (_observe_info, _step_args)
    keys = {GeneralsVecEnv: (["player_id", "turn", "valid_actions_mask"],
                             ["error", "invalid_action", "reset", "turn", "valid_actions_mask", "winner"]),
            GeneralsSelfPlayVecEnv: (["player_ids", "turn", "valid_actions_mask"],
                                     ["alive", "error", "invalid", "reset", "turn", "valid_actions_mask", "winner"])}
    for cls, (reset_keys, step_keys) in keys.items():
        env = cls(8, 8, 8, max_players=2, device_outputs=True)
        try:
            _, info = env.reset()
            assert sorted(info) == reset_keys
            act = t.zeros(info["valid_actions_mask"].shape[:-1], dtype=t.int64, device=_dev())
            _, _, _, _, info = env.step(act)
            assert sorted(info) == step_keys
            _, info = env.copy_envs([4, 5], [0, 1])
            assert sorted(info) == reset_keys
            assert env._feat_bufs is None                                # nothing allocated
        finally:
            env.close()
        env = cls(8, 8, 8, max_players=2, device_outputs=True, strategic_features=True, feature_cap=16)
        try:
            obs, info = env.reset()
            assert sorted(info) == sorted(reset_keys + ["strategic_features"])
            _check_info(obs, info, cap=16)
        finally:
            env.close()


def test_env_refuses_a_padded_batch_of_unequal_board_sizes():
    """an env of a padded batch lays its planes out with its own row pitch: the option refuses it (reset, restore_state)"""
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    env = GeneralsVecEnv(8, 10, 10, max_players=2, device_outputs=True, strategic_features=True)
    plain = GeneralsVecEnv(8, 10, 10, max_players=2, device_outputs=True)
    try:
        env.reset()
        env._check_uniform_boards()                                      # every board 10x10: accepted
        w = np.full(8, 10, np.int32)
        w[3] = 8
        for e in (env, plain):
            e.engine.reset_generated(3, width=w, height=np.full(8, 10, np.int32), players=np.full(8, 2, np.int32))
        with pytest.raises(ValueError, match="unequal board sizes"):
            env._check_uniform_boards()
        with pytest.raises(ValueError, match="unequal board sizes"):
            env.restore_state(env.save_state())
        plain._check_uniform_boards()                                    # option off: nothing is checked (or read)
    finally:
        env.close()
        plain.close()
