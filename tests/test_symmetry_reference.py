"""The numpy definition of the board symmetries (tests/_symmetry_reference.py) against the statements of
include/generals_vec.h "board symmetries": group structure, direction tables, round trips, equivariance of the legal mask
and the number of tiles whose half move is exact.  No GPU, no build."""
import numpy as np
import pytest

import _features_reference as FR
import _qtarget_reference as QR
import _symmetry_reference as SR
from generalsreinforcementlearning_amd.symmetry import inverse_symmetry, num_symmetries


def _tile_map(sym, H, W):
    """int [H * W]: g(t) per tile, read off a transformed plane of tile indices"""
    moved = SR.transform_planes(np.arange(H * W).reshape(H, W), sym).reshape(-1)      # moved[g(t)] = t
    g = np.empty(H * W, np.int64)
    g[moved] = np.arange(H * W)
    return g


def test_the_eight_maps_form_a_group_on_4x4():
    maps = [tuple(_tile_map(s, 4, 4)) for s in range(8)]
    assert len(set(maps)) == 8
    for a in range(8):
        for b in range(8):
            ab = tuple(np.asarray(maps[b])[np.asarray(maps[a])])                       # a, then b
            assert ab in maps
        inv = inverse_symmetry(a)
        assert inv == SR.INVERSE[a] == (6 if a == 5 else 5 if a == 6 else a)
        assert tuple(np.asarray(maps[inv])[np.asarray(maps[a])]) == maps[0] == tuple(range(16))
    assert num_symmetries(4, 4) == SR.num_symmetries(4, 4) == 8
    assert num_symmetries(3, 5) == SR.num_symmetries(3, 5) == 4


def test_tile_maps_follow_the_three_steps():
    for H, W in ((4, 4), (3, 5), (5, 3), (1, 1), (1, 6)):
        for s in range(SR.num_symmetries(H, W)):
            g = _tile_map(s, H, W)
            for y in range(H):
                for x in range(W):
                    gx, gy = SR.map_xy(s, x, y, W, H)
                    assert g[y * W + x] == gy * W + gx


def test_direction_tables_are_the_documented_ones():
    assert SR.DIR_TABLES == ((0, 1, 2, 3), (0, 3, 2, 1), (2, 1, 0, 3), (2, 3, 0, 1), (3, 2, 1, 0), (3, 0, 1, 2), (1, 2, 3, 0),
                             (1, 0, 3, 2))
    for s in range(8):                                                                   # ... and follow from the vectors
        for d, (dx, dy) in enumerate(QR.DIRS):
            assert QR.DIRS[SR.DIR_TABLES[s][d]] == SR.map_vector(s, dx, dy)
        # the table of the inverse is the inverse table
        assert [SR.DIR_TABLES[SR.INVERSE[s]][SR.DIR_TABLES[s][d]] for d in range(4)] == [0, 1, 2, 3]


def test_action_rows_move_tile_and_direction():
    for H, W in ((4, 4), (5, 3)):
        A = 5 * H * W
        for s in range(SR.num_symmetries(H, W)):
            g = _tile_map(s, H, W)
            row = SR.transform_action_rows(np.arange(A), s, H, W)
            for t in range(H * W):
                for d in range(5):
                    d2 = 4 if d == 4 else SR.DIR_TABLES[s][d]
                    assert row[5 * g[t] + d2] == 5 * t + d
                    assert SR.transform_actions(np.array([5 * t + d]), s, H, W)[0] == 5 * g[t] + d2
            assert list(SR.transform_actions(np.array([-1, A, A + 7, -9]), s, H, W)) == [-1, A, A + 7, -9]


@pytest.mark.parametrize("H,W", [(4, 4), (5, 3), (15, 15)])
def test_round_trips(H, W):
    rng = np.random.default_rng(H * 100 + W)
    A = 5 * H * W
    planes = rng.random((3, 9, H, W)).astype(np.float32)
    mask = rng.random((3, A)) < 0.3
    action = rng.integers(0, A, size=64)
    for s in range(SR.num_symmetries(H, W)):
        inv = inverse_symmetry(s)
        assert np.array_equal(SR.transform_planes(SR.transform_planes(planes, s), inv), planes)
        assert np.array_equal(SR.transform_action_rows(SR.transform_action_rows(mask, s, H, W), inv, H, W), mask)
        assert np.array_equal(SR.transform_actions(SR.transform_actions(action, s, H, W), inv, H, W), action)
    # the whole call: forward, then inverse=True with the original action restores every tensor, fallen-back rows included
    rows = 40
    sym = rng.integers(0, SR.num_symmetries(H, W), size=rows).astype(np.uint8)
    planes = rng.random((rows, 2, H, W)).astype(np.float32)
    mask = rng.random((rows, A)) < 0.3
    action = 5 * rng.integers(0, H * W, size=rows) + 4
    p2, m2, _, a2, applied = SR.apply(sym, H, W, [planes], mask=mask, action=action)
    p3, m3, _, _, applied3 = SR.apply(sym, H, W, p2, mask=m2, action=action, inverse=True)
    assert np.array_equal(applied, applied3) and np.array_equal(p3[0], planes) and np.array_equal(m3, mask)
    # ... and the action comes back through a forward call with the inverse of applied
    _, _, _, a3, applied4 = SR.apply(np.array([SR.INVERSE[s] for s in applied], np.uint8), H, W, action=a2)
    assert np.array_equal(a3, action) and np.array_equal(applied4, [SR.INVERSE[s] for s in applied])


@pytest.mark.parametrize("H,W", [(4, 4), (5, 3), (15, 15)])
def test_the_legal_mask_commutes_with_every_symmetry(H, W):
    obs = FR.random_obs(np.random.default_rng(7 * H + W), 12, H, W)
    mask = QR.mask_from_observation(obs)
    assert mask.any()
    for s in range(SR.num_symmetries(H, W)):
        assert np.array_equal(QR.mask_from_observation(SR.transform_planes(obs, s)), SR.transform_action_rows(mask, s, H, W)), s


def test_exact_tile_counts():
    assert [int(SR.exact_tiles(s, 4, 4).sum()) for s in range(8)] == [16, 12, 2, 2, 0, 4, 4, 6]
    assert int(SR.exact_tiles(1, 15, 15).sum()) == 210 and int(SR.exact_tiles(2, 15, 15).sum()) == 2
    for n in (4, 15):                                 # every symmetry but the identity and the pure transpose has both kinds
        for s in (1, 2, 3, 5, 6, 7):
            assert 0 < int(SR.exact_tiles(s, n, n).sum()) < n * n
        assert SR.exact_tiles(0, n, n).all()


def test_a_half_move_that_is_not_exact_falls_back_to_the_identity():
    H = W = 4
    action = np.array([5 * t + 4 for t in range(16)] + [5 * t + 1 for t in range(16)] + [-1, 80])
    for s in range(8):
        applied = SR.applied_symmetries(np.full(action.size, s, np.uint8), action, H, W)
        assert np.array_equal(applied[:16] == s, SR.exact_tiles(s, H, W) | (s == 0))
        assert (applied[16:] == s).all()                 # full moves and out-of-range actions restrict nothing
    assert list(SR.applied_symmetries(np.array([4, 7, 8, 255, 3], np.uint8), None, 3, 5)) == [0, 0, 0, 0, 3]
