"""Hand-worked cases of the match arena's episode tally against its numpy restatement (tests/_arena_reference.py): the
definition of include/generals_vec.h "match arena", one env at a time.  No GPU: what is pinned here is the reference that
tests/test_hip_arena.py then holds the kernel against bit for bit."""
import numpy as np
import pytest

from _arena_reference import TallyReference


def _step(ref, alive, terminated=False, truncated=False, winner=-1, reward=None, reset=False, land=None):
    """one step of a one-env tally; land: per column, the number of own tiles of a 4x4 observation (None: no observation)"""
    L = ref.L
    obs = None
    if land is not None:
        obs = np.zeros((1, L, 9, 4, 4), np.float32)
        obs[:, :, 1] = 1.0                                              # somebody else's everywhere ...
        for l, n in enumerate(land):
            obs[0, l, 1].reshape(-1)[:n] = 0.5                          # ... but the column's first n tiles
    ref.update(None if alive is None else np.array([alive], bool), np.array([terminated]), np.array([truncated]),
               np.array([winner], np.int8), np.array([reward if reward is not None else [0.0] * L], np.float64), np.array([reset]), obs)


def _check_invariant(ref):
    for b in range(ref.B):
        for i in range(ref.L):
            assert ref.pair2[b, i, i] == 0
            for j in range(ref.L):
                if i != j:
                    assert ref.pair2[b, i, j] + ref.pair2[b, j, i] == 2 * ref.games[b]


def test_two_player_win():
    ref = TallyReference(1, 2)
    _step(ref, [True, True], reward=[0.5, -0.25])
    _step(ref, [True, True], reward=[0.25, 0.0])
    _step(ref, [True, False], terminated=True, winner=0, reward=[1.0, -1.0])
    assert ref.games[0] == 1 and ref.len_sum[0] == 3
    assert ref.wins.tolist() == [[1, 0]] and ref.eliminated.tolist() == [[0, 1]]
    assert ref.pair2[0].tolist() == [[0, 2], [0, 0]]
    assert ref.ret_sum.tolist() == [[1.75, -1.25]]
    assert not ref.death.any() and ref.ep_len[0] == 0 and not ref.ep_return.any()      # the running state is cleared
    assert ref.events["win"] == 1
    _check_invariant(ref)


def test_four_players_two_deaths_on_one_step():
    ref = TallyReference(1, 4)
    _step(ref, [True, True, True, True])
    _step(ref, [True, False, False, True])                              # columns 1 and 2 die together on step 2
    _step(ref, [True, True, False, True])                               # a column seen alive again stays dead: first death counts
    _step(ref, [True, False, False, False], terminated=True, winner=0)  # column 3 dies on step 4, column 0 wins
    assert ref.eliminated.tolist() == [[0, 1, 1, 1]] and ref.wins.tolist() == [[1, 0, 0, 0]]
    assert ref.pair2[0].tolist() == [[0, 2, 2, 2],                      # the winner beats everybody
                                     [0, 0, 1, 0],                      # 1 ties with 2, behind 3 and 0
                                     [0, 1, 0, 0],
                                     [0, 2, 2, 0]]                      # the later death beats both
    assert ref.events["same_step_deaths"] == 1
    _check_invariant(ref)


def test_truncation_ranks_survivors_by_land():
    ref = TallyReference(1, 3)
    _step(ref, [True, True, True], land=[9, 9, 9])                      # land of an ordinary step is not read
    _step(ref, [True, True, False], land=[1, 2, 16])
    _step(ref, [True, True, False], truncated=True, land=[3, 7, 16])    # the dead column's land counts for nothing
    assert ref.pair2[0].tolist() == [[0, 0, 2], [2, 0, 2], [0, 0, 0]]
    assert ref.wins.tolist() == [[0, 0, 0]] and ref.eliminated.tolist() == [[0, 0, 1]] and ref.len_sum[0] == 3
    assert ref.events["trunc_distinct_land"] == 1 and ref.events["trunc_equal_land"] == 0
    _step(ref, [True, True, True], reset=True)
    _step(ref, [True, True, True], truncated=True, land=[5, 5, 4])      # equal land ties
    assert ref.pair2[0].tolist() == [[0, 1, 4], [3, 0, 4], [0, 0, 0]]
    assert ref.events["trunc_equal_land"] == 1 and ref.games[0] == 2 and ref.len_sum[0] == 4
    _check_invariant(ref)


def test_truncation_without_observation_ties_survivors():
    ref = TallyReference(1, 2)
    _step(ref, [True, True], truncated=True)
    assert ref.pair2[0].tolist() == [[0, 1], [1, 0]]
    _check_invariant(ref)


def test_termination_wins_over_truncation():
    ref = TallyReference(1, 2)
    _step(ref, [True, True], terminated=True, truncated=True, winner=1, land=[16, 1])   # both survive in `alive`: the land is ignored
    assert ref.pair2[0].tolist() == [[0, 1], [1, 0]] and ref.wins.tolist() == [[0, 1]]
    assert ref.events["term_and_trunc"] == 1
    _check_invariant(ref)


def test_winner_outside_the_learners():
    ref = TallyReference(1, 2, player_ids=[1, 3])
    _step(ref, [True, False])
    _step(ref, [False, False], terminated=True, winner=2)               # player 2 is the on-device agent
    assert ref.wins.tolist() == [[0, 0]] and ref.eliminated.tolist() == [[1, 1]]
    assert ref.pair2[0].tolist() == [[0, 2], [0, 0]]                    # column 0 lasted a step longer
    assert ref.events["outside_winner"] == 1
    ref2 = TallyReference(1, 2, player_ids=[1, 3])
    _step(ref2, [True, False], terminated=True, winner=1)               # the id, not the column index, is compared
    assert ref2.wins.tolist() == [[1, 0]]
    _check_invariant(ref)
    _check_invariant(ref2)


def test_reset_in_mid_episode_counts_nothing():
    ref = TallyReference(1, 2)
    _step(ref, [True, False], reward=[1.0, 1.0])
    _step(ref, [True, True], reset=True, terminated=True, winner=0, reward=[9.0, 9.0])   # a re-deal step: its other outputs are not read
    assert ref.games[0] == 0 and not ref.pair2.any() and not ref.ret_sum.any()
    assert not ref.death.any() and ref.ep_len[0] == 0 and not ref.ep_return.any()
    assert ref.events["reset_mid_episode"] == 1
    _step(ref, [True, True], reward=[0.5, 0.5])
    _step(ref, [False, True], terminated=True, winner=1, reward=[0.0, 1.0])
    assert ref.len_sum[0] == 2 and ref.ret_sum.tolist() == [[0.5, 1.5]] and ref.eliminated.tolist() == [[1, 0]]
    _check_invariant(ref)


def test_cap_ignores_later_games():
    ref = TallyReference(1, 2, games_cap=2)
    for winner in (0, 1):
        _step(ref, [winner == 0, winner == 1], terminated=True, winner=winner, reward=[1.0, 2.0])
        _step(ref, [True, True], reset=True)
    before = {k: v.copy() for k, v in ref.state().items()}
    _step(ref, [True, True], reward=[3.0, 3.0])
    _step(ref, [True, False], terminated=True, winner=0, reward=[1.0, 1.0])              # the third game
    assert ref.events["capped"] == 1 and ref.games[0] == 2
    for k, v in ref.state().items():
        assert np.array_equal(v, before[k]), k                          # totals unchanged, running state cleared
    _check_invariant(ref)


def test_single_learner_without_alive():
    ref = TallyReference(1, 1)
    _step(ref, None, reward=[0.25])
    _step(ref, None, terminated=True, winner=0, reward=[0.5])
    _step(ref, None, reset=True)
    _step(ref, None, terminated=True, winner=1)                         # lost: but nobody is ever recorded as eliminated
    assert ref.games[0] == 2 and ref.wins.tolist() == [[1]] and ref.eliminated.tolist() == [[0]]
    assert ref.len_sum[0] == 3 and ref.ret_sum.tolist() == [[0.75]] and ref.pair2.tolist() == [[[0]]]
    _check_invariant(ref)


@pytest.mark.parametrize("B,L,HW,cap", [(1, 2, (5, 5), 0), (5, 3, (9, 9), 2), (9, 1, None, 0)])
def test_invariant_on_scripted_sequences(B, L, HW, cap):
    from _arena_reference import feed, scripted_steps
    ref = TallyReference(B, L, games_cap=cap)
    steps, pool = scripted_steps(B, L, HW, 60, seed=3, with_alive=L > 1)
    for s in steps:
        feed(ref, s, pool)
        _check_invariant(ref)
    assert ref.games.sum() > 0
    if cap:
        assert ref.games.max() <= cap
