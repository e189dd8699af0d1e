"""The numpy restatement of the masked Q targets (tests/_qtarget_reference.py) against what it restates: the legal set of an
observation against the reference GeneralsEnv's own recorded masks and against _gym_reference.valid_actions_mask, the
argmax rule, and the properties of the categorical projection.  No GPU: this is what pins the checker of test_hip_qtarget.py."""
import json
import os

import numpy as np

import _gym_env_fixtures as F
import _gym_reference as G
import _qtarget_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gym_env_fixtures.json")) as f:
    FX = json.load(f)


def test_every_recorded_observation_gives_the_recorded_mask():
    """every reset and step of every recorded episode: the mask the reference's GeneralsEnv returned is a function of the
    observation it returned with it"""
    pairs, empty, sizes = 0, 0, set()
    for g in FX["episodes"]:
        w, h = g["w"], g["h"]
        for s in [g["reset"]] + list(g["steps"]):
            obs, want = F.decode_obs(s["obs"], w, h), F.decode_mask(s["mask"], w, h)
            got = R.mask_from_observation(obs)
            assert got.dtype == bool and got.shape == (w * h * 5,)
            assert np.array_equal(got, want), (g["name"], np.flatnonzero(got != want)[:8])
            pairs += 1
            empty += not want.any()
            sizes.add((w, h, bool(g["fog"])))
    assert pairs == 145 and empty >= 1
    assert {(7, 5), (8, 8), (15, 15), (20, 20)} == {s[:2] for s in sizes} and (8, 8, True) in sizes and (8, 8, False) in sizes


def test_random_views_agree_with_the_gym_reference():
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (1, 7), (7, 1), (7, 5), (15, 15), (32, 32)):
        n, B = w * h, 40
        owner = rng.integers(-1, 3, (B, n)).astype(np.int32)
        army = np.where(owner >= 0, rng.integers(0, 5, (B, n)) ** 3, 0).astype(np.int64)        # 0, 1, 8, 27, 64
        typ = rng.choice([0, 0, 0, 1, 2, 3], (B, n)).astype(np.int32)
        view = {"owner": owner, "army": army, "type": typ, "visible": np.ones((B, n), bool)}
        for player in (0, 2):
            obs = G.build_observation(view, player, 3, 500, w, h)
            want = G.valid_actions_mask(view, player, w, h)
            assert np.array_equal(R.mask_from_observation(obs), want), (w, h, player)


def _obs(h, w, own=(), army=None, mountains=(), enemy=()):
    """a [9, h, w] observation: own / enemy / mountains are (y, x) lists, army {(y, x): count}"""
    o = np.zeros((9, h, w), np.float32)
    for y, x in own:
        o[1, y, x] = 0.5
    for y, x in enemy:
        o[1, y, x] = 1.0
    for (y, x), a in (army or {}).items():
        o[2, y, x] = np.float32(np.log(a + 1) / 10.0)
    for y, x in mountains:
        o[4, y, x] = 1.0
    return o


def _legal(o):
    h, w = o.shape[1:]
    return sorted((int(i) // 5 // w, int(i) // 5 % w, int(i) % 5) for i in np.flatnonzero(R.mask_from_observation(o)))


def test_hand_written_boards():
    h, w = 4, 5
    for (y, x), dirs in {(0, 0): (1, 2), (0, 4): (2, 3), (3, 0): (0, 1), (3, 4): (0, 3),       # the corners
                         (0, 2): (1, 2, 3), (3, 2): (0, 1, 3), (1, 0): (0, 1, 2), (2, 4): (0, 2, 3),   # the edges
                         (1, 2): (0, 1, 2, 3)}.items():
        o = _obs(h, w, own=[(y, x)], army={(y, x): 5})
        assert _legal(o) == sorted([(y, x, d) for d in dirs] + [(y, x, 4)]), (y, x)
    # a mountain neighbour: that direction goes, the rest stays; mountains all around: nothing, the half move included
    o = _obs(h, w, own=[(1, 2)], army={(1, 2): 9}, mountains=[(0, 2)])
    assert _legal(o) == [(1, 2, 1), (1, 2, 2), (1, 2, 3), (1, 2, 4)]
    o = _obs(h, w, own=[(1, 2)], army={(1, 2): 9}, mountains=[(0, 2), (1, 3), (2, 2), (1, 1)])
    assert _legal(o) == []
    # armies of exactly 1 and exactly 2
    assert _legal(_obs(h, w, own=[(1, 2)], army={(1, 2): 1})) == []
    assert len(_legal(_obs(h, w, own=[(1, 2)], army={(1, 2): 2}))) == 5
    assert np.float32(np.log(2) / 10) < np.float32(0.09) < np.float32(np.log(3) / 10)
    # an enemy tile with a large army is no source; an own tile next to it may move onto it
    o = _obs(h, w, own=[(1, 1)], enemy=[(1, 2)], army={(1, 1): 3, (1, 2): 1000})
    assert {t[:2] for t in _legal(o)} == {(1, 1)} and (1, 1, 1) in _legal(o)
    # 1x1: no neighbour on the board; 1x7: left and right only
    assert _legal(_obs(1, 1, own=[(0, 0)], army={(0, 0): 50})) == []
    o = _obs(1, 7, own=[(0, 0), (0, 3), (0, 6)], army={(0, 0): 2, (0, 3): 2, (0, 6): 2})
    assert _legal(o) == [(0, 0, 1), (0, 0, 4), (0, 3, 1), (0, 3, 3), (0, 3, 4), (0, 6, 3), (0, 6, 4)]
    o = _obs(7, 1, own=[(0, 0), (6, 0)], army={(0, 0): 2, (6, 0): 2})
    assert _legal(o) == [(0, 0, 2), (0, 0, 4), (6, 0, 0), (6, 0, 4)]
    # no step wraps from the last column to the first of the next row
    o = _obs(2, 3, own=[(0, 2)], army={(0, 2): 4}, mountains=[(1, 2), (0, 1)])
    assert _legal(o) == []


def test_argmax_rule():
    inf, nan = np.inf, np.nan
    v = np.array([[1.0, 5.0, 5.0, 9.0], [-inf, -inf, -inf, -inf], [nan, 2.0, nan, 2.0], [nan, nan, 1.0, nan], [3.0, 1.0, 2.0, 0.0],
                  [nan, -inf, 7.0, -inf]], np.float32)
    m = np.array([[1, 1, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1], [1, 1, 0, 1], [0, 0, 0, 0], [1, 1, 0, 1]], bool)
    #            tie: lowest   all -inf: lowest legal   NaN never wins   only NaN: nothing   nothing legal   NaN, then -inf
    assert R.masked_argmax(v, m).tolist() == [1, 1, 1, -1, -1, 1]


def _one_own_tile(rows, h=3, w=3):
    o = np.zeros((rows, 9, h, w), np.float32)
    o[:, 1, 1, 1], o[:, 2, 1, 1] = 0.5, np.float32(np.log(6) / 10)
    return o


def test_scalar_target_is_one_multiply_and_one_add_in_float32():
    rows, A = 6, 45
    rng = np.random.default_rng(2)
    o = _one_own_tile(rows)
    o[5, 1] = 0                                                                          # row 5: nothing legal
    q = rng.standard_normal((rows, A)).astype(np.float32)
    sel = rng.standard_normal((rows, A)).astype(np.float32)
    r = rng.standard_normal(rows).astype(np.float32)
    disc = np.array([0.99, 0.5, 0.970299, 0.9, 0.9, 0.9], np.float32)
    done = np.array([0, 0, 0, 1, 0, 0], bool)
    t, a, nv = R.q_target(o, q, r, disc, done, q_select=sel)
    legal = np.arange(20, 25)                                                            # tile 4's five actions
    for i in range(rows):
        if i == 5:
            assert a[i] == -1 and nv[i] == 0 and t[i] == r[i]
            continue
        assert a[i] == legal[np.argmax(sel[i, legal])]
        if done[i]:
            assert nv[i] == 0 and t[i] == r[i]
        else:
            assert nv[i] == q[i, a[i]] and t[i] == np.float32(r[i] + np.float32(disc[i] * q[i, a[i]]))
    t2, a2, _ = R.q_target(o, q, r, 0.99, done)                                          # scalar gamma, no selection network
    assert a2[0] == legal[np.argmax(q[0, legal])] and t2[0] == np.float32(r[0] + np.float32(np.float32(0.99) * q[0, a2[0]]))
    garbage = np.where(R.mask_from_observation(o), sel, np.nan).astype(np.float32)       # illegal entries change nothing
    t3, a3, nv3 = R.q_target(o, np.where(R.mask_from_observation(o), q, 1e30).astype(np.float32), r, disc, done, q_select=garbage)
    assert np.array_equal(t3, t) and np.array_equal(a3, a) and np.array_equal(nv3, nv)


def test_projection_properties():
    rows, N, lo, hi = 64, 51, -10.0, 10.0
    rng = np.random.default_rng(3)
    o = _one_own_tile(rows)
    logits = (2 * rng.standard_normal((rows, 45, N))).astype(np.float32)
    r = (4 * rng.standard_normal(rows)).astype(np.float32)
    r[:4] = (-250.0, 250.0, -10.0, 10.0)                                                 # beyond either bound, and on them
    disc = np.full(rows, 0.99, np.float32)
    done = np.zeros(rows, bool)
    done[8:16] = True
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 2e-6)):
        m, a = R.categorical_target(o, logits, r, disc, done, lo, hi, dtype=dtype)
        assert m.dtype == dtype and m.shape == (rows, N) and (m >= 0).all()
        assert np.abs(m.sum(1) - 1).max() <= tol
        assert (a[done] == -1).all() and (a[~done] >= 20).all() and (a[~done] < 25).all()
        assert m[0, 0] > 0.98 and m[1, N - 1] > 0.98                                     # clamped support: nearly all mass at the bound
        # a done row is the point mass at the reward, split between its two neighbours on the support
        for i in range(8, 16):
            b = (np.clip(float(r[i]), lo, hi) - lo) / ((hi - lo) / (N - 1))
            want = np.maximum(0, 1 - np.abs(b - np.arange(N)))
            assert np.abs(m[i] - want).max() <= 4e-6
        # discount 0 is done
        m0, _ = R.categorical_target(o, logits, r, np.zeros(rows, np.float32), np.zeros(rows, bool), lo, hi, dtype=dtype)
        md, _ = R.categorical_target(o, logits, r, disc, np.ones(rows, bool), lo, hi, dtype=dtype)
        assert np.abs(m0 - md).max() <= tol
    # an atom landing exactly on a support point: reward 0.4 * 3, discount 1 moves every atom three atoms up, the top three
    # clamp onto the last
    m, a = R.categorical_target(o, logits, np.full(rows, 1.2, np.float32), np.ones(rows, np.float32), np.zeros(rows, bool), lo, hi)
    p = R._softmax(logits[np.arange(rows), a].astype(np.float64))
    want = np.zeros((rows, N))
    want[:, 3:] = p[:, :N - 3]
    want[:, N - 1] += p[:, N - 3:].sum(1)
    assert np.abs(m - want).max() <= 1e-6                                                # float32(1.2) is 1.2 to 5e-8
    # Double: the selection network picks, the evaluation network is projected
    sel = (2 * rng.standard_normal((rows, 45, N))).astype(np.float32)
    m2, a2 = R.categorical_target(o, logits, r, disc, done, lo, hi, logits_select=sel)
    q = R.categorical_q(o, sel, lo, hi)[0]
    assert np.array_equal(a2[~done], q.argmax(1)[~done])
    i = int(np.flatnonzero(~done & (a2 != a))[0])
    want = R.project(R._softmax(logits[i:i + 1, a2[i]].astype(np.float64)), r[i:i + 1].astype(np.float64), disc[i:i + 1].astype(np.float64), lo, hi)
    assert np.abs(m2[i] - want[0]).max() <= 1e-12
