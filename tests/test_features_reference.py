"""Pins tests/_features_reference.py - the numpy restatement of the strategic feature planes that the HIP kernel is compared
with bit for bit (tests/test_hip_features.py) - on boards small enough to work out by hand.  Expected arrays are literals."""
import numpy as np

import _features_reference as R

ONES = lambda h, w: np.ones((h, w), np.float32)


def _b(rows):
    """'#.x' pictures -> bool map of the '#' tiles"""
    return np.array([[c == "#" for c in r] for r in rows], bool)


def test_3x3_with_a_centre_mountain():
    gen = _b(["#..", "...", "..."])
    obs = R.make_obs(3, 3, mtn=_b(["...", ".#.", "..."]), gen=gen, mine=_b(["#..", "..#", "..."]), enemy=_b(["...", "...", "..#"]))
    f = R.features_one(obs, cap=8)
    assert f.dtype == np.float32 and f.shape == (5, 3, 3)
    np.testing.assert_array_equal(f[0], np.array([[0, 1, 2], [1, 8, 3], [2, 3, 4]], np.float32) / 8)    # the walk goes round the mountain
    np.testing.assert_array_equal(f[1], np.array([[4, 3, 2], [3, 8, 1], [2, 1, 0]], np.float32) / 8)
    np.testing.assert_array_equal(f[2], ONES(3, 3))                                                       # no city
    np.testing.assert_array_equal(f[3], ONES(3, 3))                                                       # no fog
    np.testing.assert_array_equal(f[4], np.array([[0, 0, 0], [0, 0, 1], [0, 0, 0]], np.float32))       # (1, 2) touches the enemy at (2, 2)


def test_1x5_corridor():
    obs = R.make_obs(1, 5, enemy=_b(["....#"]), vis=_b([".####"]))
    f = R.features_one(obs, cap=4)
    np.testing.assert_array_equal(f[1], np.array([[1.0, 0.75, 0.5, 0.25, 0.0]], np.float32))             # d = 4 saturates at cap = 4
    np.testing.assert_array_equal(f[3], np.array([[0.0, 0.25, 0.5, 0.75, 1.0]], np.float32))
    np.testing.assert_array_equal(f[0], ONES(1, 5))
    np.testing.assert_array_equal(f[4], np.zeros((1, 5), np.float32))
    g = R.features_one(obs, cap=2)
    np.testing.assert_array_equal(g[1], np.array([[1.0, 1.0, 1.0, 0.5, 0.0]], np.float32))


def test_a_step_never_wraps_from_the_last_column_to_the_next_row():
    obs = R.make_obs(2, 4, enemy=_b(["...#", "...."]))
    f = R.features_one(obs, cap=8)
    # (1, 0) follows (0, 3) in memory: its distance is W = 4, not 1
    np.testing.assert_array_equal(f[1], np.array([[3, 2, 1, 0], [4, 3, 2, 1]], np.float32) / 8)
    obs = R.make_obs(2, 4, enemy=_b(["....", "#..."]))
    f = R.features_one(obs, cap=8)
    np.testing.assert_array_equal(f[1], np.array([[1, 2, 3, 4], [0, 1, 2, 3]], np.float32) / 8)         # and (0, 3) is not next to (1, 0)


def test_an_empty_source_set_gives_ones():
    obs = R.make_obs(4, 3, mtn=_b(["#..", "...", "...", "..#"]))
    f = R.features_one(obs, cap=64)
    np.testing.assert_array_equal(f[:4], np.ones((4, 4, 3), np.float32))
    np.testing.assert_array_equal(f[4], np.zeros((4, 3), np.float32))


def test_a_source_enclosed_by_mountains_reaches_nothing():
    obs = R.make_obs(3, 3, mtn=_b([".#.", "#.#", ".#."]), enemy=_b(["...", ".#.", "..."]))
    f = R.features_one(obs, cap=64)
    want = ONES(3, 3)
    want[1, 1] = 0.0
    np.testing.assert_array_equal(f[1], want)


def test_a_source_on_an_impassable_tile_is_no_source():
    """both ends of a path are passable: an enemy mark on a mountain starts nothing"""
    obs = R.make_obs(1, 3, mtn=_b(["#.."]), enemy=_b(["#.."]))
    np.testing.assert_array_equal(R.features_one(obs, cap=4)[1], ONES(1, 3))


def test_cities_to_take_and_fog():
    obs = R.make_obs(1, 4, city=_b(["#..#"]), mine=_b(["#..."]), vis=_b(["###."]), mtn=_b(["...."]))
    f = R.features_one(obs, cap=4)
    np.testing.assert_array_equal(f[2], np.array([[0.75, 0.5, 0.25, 0.0]], np.float32))                  # the own city at x = 0 is no target
    np.testing.assert_array_equal(f[3], np.array([[0.75, 0.5, 0.25, 0.0]], np.float32))
    fogged_mountain = R.make_obs(1, 3, mtn=_b(["#.."]), vis=_b([".##"]))
    np.testing.assert_array_equal(R.features_one(fogged_mountain, cap=4)[3], ONES(1, 3))                 # !vis & pass: a fogged mountain is no target


def test_9x9_serpentine():
    obs = R.serpentine(9)
    dist, _ = R.distances_one(obs)
    assert dist[0].max() == 48 and dist[0, 8, 8] == 48 and dist[0, 8, 0] == 40 and dist[0, 0, 8] == 8 and dist[0, 1, 8] == 9 and dist[0, 2, 8] == 10
    f = R.features_one(obs, cap=32)
    passable = obs[4] == 0
    assert int((f[0][passable] == 1.0).sum()) == 17                    # d = 32 .. 48
    assert f[0, 0, 0] == 0.0 and f[0, 0, 1] == np.float32(1 / 32)
    np.testing.assert_array_equal(f[0][~passable], 1.0)


def test_32x32_serpentine_depth():
    assert R.max_depth(R.serpentine(32)) == 527


def test_batched_form_and_cap():
    rng = np.random.default_rng(5)
    obs = R.random_obs(rng, 3, 6, 7)
    f = R.features(obs.reshape(3, 1, 9, 6, 7), cap=16)
    assert f.shape == (3, 1, 5, 6, 7)
    for i in range(3):
        np.testing.assert_array_equal(f[i, 0], R.features_one(obs[i], cap=16))
    vals = np.unique(f[:, :, :4] * 16)
    assert np.all(vals == np.rint(vals)) and vals.min() >= 0 and vals.max() <= 16


def test_level_by_level_form_equals_the_queue_search():
    rng = np.random.default_rng(9)
    for H, W, share in ((5, 5, 0.2), (15, 15, 0.2), (15, 15, 0.45), (3, 32, 0.2), (32, 32, 0.45)):
        obs = R.random_obs(rng, 6, H, W, mountain_share=share)
        for cap in (2, 64, 1024):
            np.testing.assert_array_equal(R.features_batch(obs.reshape(3, 2, 9, H, W), cap), R.features(obs, cap).reshape(3, 2, 5, H, W))
    for n, cap in ((9, 32), (32, 1024)):
        np.testing.assert_array_equal(R.features_batch(R.serpentine(n), cap), R.features_one(R.serpentine(n), cap))
