"""The host side of the match arena (generalsreinforcementlearning_amd/arena.py): seating, the rating fit, and the argument
checks of EpisodeTally.update and gvec_arena_update.  The file runs with and without a device and the entry point's pointers
are placeholders, so every call of it goes through tests/_api_calls.py, which launches nothing on them."""
import ctypes as C

import numpy as np
import pytest

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


# ---- seating ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_,E", [(2, 2), (2, 3), (4, 2), (4, 5), (3, 3)])
def test_balanced_seating_is_balanced_over_one_period(L_, E):
    from generalsreinforcementlearning_amd.arena import balanced_seating, seating_period
    period = seating_period(L_, E)
    seat = balanced_seating(period, L_, E)
    assert seat.shape == (period, L_) and seat.dtype == np.int64
    rows = [tuple(r) for r in seat]
    assert rows == sorted(set(rows))                                    # distinct selections, in lexicographic order
    for r in rows:
        assert len(set(r)) == min(L_, E)                                # E >= L: no repetition; E < L: every entrant is used
    for c in range(L_):
        counts = np.bincount(seat[:, c], minlength=E)
        assert (counts == period // E).all(), (c, counts)               # every entrant in every column equally often
    twice = balanced_seating(2 * period + 1, L_, E)                     # the table cycles
    assert np.array_equal(twice[:period], seat) and np.array_equal(twice[period:2 * period], seat) and np.array_equal(twice[-1], seat[0])
    assert seating_period(L_, E) == {(2, 2): 2, (2, 3): 6, (4, 2): 14, (4, 5): 120, (3, 3): 6}[(L_, E)]


# ---- ratings ---------------------------------------------------------------------------------------------------------------
def test_fit_elo_two_entrants_is_the_closed_form():
    from generalsreinforcementlearning_amd.arena import expected_score, fit_elo
    for w_ab, w_ba, prior in ((30.0, 10.0, 1.0), (7.5, 2.5, 0.0), (12.0, 0.0, 1.0), (3.0, 3.0, 2.0)):
        n = w_ab + w_ba
        r = fit_elo([[0, w_ab], [w_ba, 0]], [[0, n], [n, 0]], prior_draws=prior)
        want = 400.0 * np.log10((w_ab + 0.5 * prior) / (w_ba + 0.5 * prior))
        assert abs((r[0] - r[1]) - want) < 1e-9, (w_ab, w_ba, prior, r)
        assert r[0] == 1500.0
        assert abs(expected_score(r[0], r[1]) - (w_ab + 0.5 * prior) / (n + prior)) < 1e-12
    assert expected_score(1500.0, 1500.0) == 0.5 and abs(expected_score(1900.0, 1500.0) - 10.0 / 11.0) < 1e-15


def test_fit_elo_meets_the_likelihood_condition():
    from generalsreinforcementlearning_amd.arena import expected_score, fit_elo
    rng = np.random.default_rng(0)
    E, prior = 4, 1.0
    games = np.triu(rng.integers(5, 40, size=(E, E)), 1).astype(np.float64)
    games = games + games.T
    share = np.triu(rng.integers(0, 5, size=(E, E)) / 4.0, 1)          # ties included: halves of games
    score = games * (share + np.tril(1.0 - share.T, -1))
    assert np.allclose(score + score.T, games)
    r = fit_elo(score, games, prior_draws=prior)
    n = games + prior * (1 - np.eye(E))
    W = score.sum(1) + 0.5 * prior * (E - 1)
    exp = expected_score(r[:, None], r[None, :])
    assert np.abs((n * exp).sum(1) - W).max() < 1e-8
    # the order of the entrants plays no part
    perm = np.array([2, 0, 3, 1])
    rp = fit_elo(score[np.ix_(perm, perm)], games[np.ix_(perm, perm)], anchor=1, prior_draws=prior)
    assert np.abs(rp - r[perm]).max() < 1e-6


def test_fit_elo_undefeated_entrant_and_anchor():
    from generalsreinforcementlearning_amd.arena import fit_elo
    score = np.array([[0, 20, 20], [0, 0, 12], [0, 8, 0]], np.float64)      # entrant 0 never lost
    games = np.array([[0, 20, 20], [20, 0, 20], [20, 20, 0]], np.float64)
    r = fit_elo(score, games)
    assert np.isfinite(r).all() and r[0] > r[1] > r[2] and r[0] == 1500.0
    r2 = fit_elo(score, games, anchor=2, anchor_rating=1000.0)
    assert r2[2] == 1000.0 and np.abs((r2 - r2[2]) - (r - r[2])).max() < 1e-6
    with pytest.raises(ValueError, match="prior_draws"):
        fit_elo(score, games, prior_draws=0.0)                           # without the prior its strength has no maximum
    with pytest.raises(ValueError):
        fit_elo(score, games[:2, :2])
    with pytest.raises(ValueError, match="anchor"):
        fit_elo(score, games, anchor=3)


# ---- EpisodeTally.update: every refusal comes before any launch --------------------------------------------------------------
def test_python_front_rejects_bad_input_before_any_launch():
    import torch
    from generalsreinforcementlearning_amd import EpisodeTally
    for bad in (0, 9):
        with pytest.raises(ValueError, match="num_learners"):
            EpisodeTally(4, bad)
    with pytest.raises(TypeError):
        EpisodeTally(4.0, 2)
    with pytest.raises(ValueError, match="player_ids"):
        EpisodeTally(4, 2, player_ids=[0, 1, 2])
    with pytest.raises(ValueError, match="games_cap"):
        EpisodeTally(4, 2, games_cap=-1)
    with pytest.raises(ValueError, match="CUDA"):
        EpisodeTally(4, 2, device="cpu")
    t = EpisodeTally(4, 2)                                               # allocates nothing: fine without a device
    good = dict(alive=torch.ones(4, 2, dtype=torch.bool), terminated=torch.zeros(4, dtype=torch.bool),
                truncated=torch.zeros(4, dtype=torch.bool), winner=torch.zeros(4, dtype=torch.int8),
                reward=torch.zeros(4, 2, dtype=torch.float64), reset=torch.zeros(4, dtype=torch.bool), obs=torch.zeros(4, 2, 9, 5, 5))
    with pytest.raises(ValueError, match="CUDA"):
        t.update(**good)                                                 # CPU tensors
    for name, wrong, text in (("alive", torch.ones(4, 2), "bool or uint8"), ("terminated", torch.zeros(4), "bool or uint8"),
                              ("truncated", torch.zeros(4, dtype=torch.int32), "bool or uint8"),
                              ("reset", torch.zeros(4, dtype=torch.int64), "bool or uint8"),
                              ("winner", torch.zeros(4, dtype=torch.int64), "int8"), ("reward", torch.zeros(4, 2), "float64"),
                              ("obs", torch.zeros(4, 2, 9, 5, 5, dtype=torch.float64), "float32"),
                              ("terminated", None, "torch.Tensor"), ("winner", [0, 0, 0, 0], "torch.Tensor")):
        with pytest.raises(TypeError, match=text):
            t.update(**{**good, name: wrong})
    for name, shape in (("alive", (4, 3)), ("alive", (8,)), ("terminated", (3,)), ("truncated", (4, 1)), ("reset", (5,)), ("winner", (4, 2)),
                        ("reward", (4,)), ("reward", (2, 4))):
        with pytest.raises(ValueError, match="is not"):
            t.update(**{**good, name: torch.zeros(shape, dtype=good[name].dtype)})
    for shape in ((4, 2, 8, 5, 5), (8, 9, 5, 5), (4, 3, 9, 5, 5), (4, 2, 9, 5, 33)):
        with pytest.raises(ValueError):
            t.update(**{**good, "obs": torch.zeros(shape)})
    assert t._state is None                                              # still nothing allocated


def test_struct_layout_matches_the_header():
    f = lib.ArenaArgs
    assert C.sizeof(f) == 32 + 17 * 8
    assert (f.rows.offset, f.width.offset, f.height.offset, f.num_learners.offset, f.games_cap.offset, f.obs_row_stride.offset,
            f.alive.offset, f.obs.offset, f.death.offset, f.pair2.offset) == (0, 8, 12, 16, 20, 24, 32, 88, 96, 160)


FN = "gvec_arena_update"
P = 1 << 20   # stands for a device pointer: no check dereferences it, a launch would (passes_checks keeps it from one)
STATE = ("death", "ep_len", "ep_return", "games", "wins", "eliminated", "len_sum", "ret_sum", "pair2")


def _args(**over):
    kw = dict(rows=3, width=15, height=15, num_learners=2, games_cap=0, obs_row_stride=9 * 225, alive=P, terminated=P, truncated=P, reset=P,
              winner=P, reward=P, player_ids=P, obs=P, **{k: P for k in STATE})
    kw.update(over)
    return lib.ArenaArgs(**kw)


def _rejected(L, a, text):
    rejected(L, FN, a, text)


def test_entry_point_refuses_bad_arguments_without_a_gpu(L):
    _rejected(L, None, "NULL")
    for k in STATE + ("terminated", "truncated", "winner", "reward", "player_ids"):
        _rejected(L, _args(**{k: None}), "NULL")
        _rejected(L, _args(rows=0, **{k: None}), "NULL")                 # the checks come first all the same
    for n in (9, 0, -1):
        _rejected(L, _args(num_learners=n), f"num_learners {n} outside [1, 8]")
    _rejected(L, _args(rows=-1), "rows -1")
    _rejected(L, _args(rows=2 ** 31), "rows")
    _rejected(L, _args(games_cap=-2), "games_cap -2")
    _rejected(L, _args(width=33), "width 33")
    _rejected(L, _args(height=0), "height 0")
    _rejected(L, _args(obs_row_stride=9 * 225 - 1), "obs_row_stride")


def test_zero_rows_is_a_no_op_without_a_device(L):
    passes_checks(L, FN, _args(rows=0))
    passes_checks(L, FN, _args(rows=0, num_learners=8, games_cap=5, alive=None, reset=None))
    # without an observation the board is not read: its fields may hold anything
    passes_checks(L, FN, _args(rows=0, obs=None, width=0, height=99, obs_row_stride=0, num_learners=1))


def test_passing_arguments_reach_the_device_check(L):
    """what refuses a call that passes every check on a box without a GPU is the device, with another code (with one, the
    stand-in pointers must not be launched on: passes_checks makes no call there)"""
    passes_checks(L, FN, _args())                                        # GVEC_E_NO_DEVICE
    passes_checks(L, FN, _args(alive=None, reset=None, obs=None, width=0, height=0))
