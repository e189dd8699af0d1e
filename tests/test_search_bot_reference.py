"""The CPU reference of the playout search with scripted-opponent playouts (tests/_search_bot_reference.py) against its own
definition: no GPU.  On the coverage roots of tests/_search_reference.py - 5x5 two-player games old enough to end inside a
playout - the reference with no seat on the rule is the agent search's reference, and with seats on it the run takes both
branches of the rule (captures and consolidation), ends playouts in every way, and mixes in the agent's moves."""
import numpy as np
import pytest

import _bot_reference as BR
import _search_bot_reference as SBR
import _search_reference as SR

W, H, P = SR.COVER_W, SR.COVER_H, SR.COVER_P
K, R, D, SEED = SR.COVER_K, 2, 4, SR.COVER_SEARCH_SEED


def _terms(fog, bot_players, permille=0, depth=D, replicas=R):
    st, players, cand = SR.coverage_roots(fog)
    return SBR.reference_terms_bot(st, None, players, cand, replicas, depth, SEED, W, H, P, bot_players, permille, fog=fog)


def test_no_seat_on_the_rule_is_the_agent_reference():
    st, players, cand = SR.coverage_roots(True)
    want = SR.reference_terms(st, None, players, cand, R, D, SEED, W, H, P, fog=True)
    got = _terms(True, 0)
    assert (want[..., 0] == 1).any() and (want[..., 3] == 1).any()
    assert np.array_equal(got, want)
    # ... at the agent search's own depth and replicas too, where games end inside the playouts
    deep = SR.reference_terms(st, None, players, cand, SR.COVER_R, SR.COVER_D, SEED, W, H, P, fog=True)
    assert np.array_equal(_terms(True, 0, depth=SR.COVER_D, replicas=SR.COVER_R), deep)


@pytest.mark.parametrize("fog,bot_players,permille,depth", [(True, 0b11, 0, D), (False, 0b11, 100, D), (True, 0b10, 0, 8)],
                         ids=["fog_both", "nofog_both_mix100", "fog_seat1_depth8"])
def test_both_branches_of_the_rule_and_every_outcome_occur(monkeypatch, fog, bot_players, permille, depth):
    """bot_move is wrapped: a returned move whose target tile the seat owns is a consolidation (BFS) step, any other a capture."""
    counts = {"capture": 0, "consolidation": 0, "none": 0}
    inner = BR.bot_move

    def counted(v):
        mv = inner(v)
        if mv is None:
            counts["none"] += 1
        else:
            own = v.seen[mv[3] * v.w + mv[2]] and v.owner[mv[3] * v.w + mv[2]] == v.p
            counts["consolidation" if own else "capture"] += 1
        return mv

    monkeypatch.setattr(BR, "bot_move", counted)
    terms = _terms(fog, bot_players, permille, depth)
    assert counts["capture"] >= 1 and counts["consolidation"] >= 1, counts
    valid = terms[..., 0] == 1
    assert (terms[..., 3] == 1).any(), "no playout is won"
    assert (valid & (terms[..., 2] == 0)).any(), "no playout ends with the seat dead"
    assert (valid & (terms[..., 1] < depth)).any(), "no playout ends before its depth"
    assert (terms[..., 1] <= depth).all() and (terms[valid][:, 1] >= 1).all()
    assert ((terms[..., 3] == 0) | (terms[..., 2] == 1)).all()               # the winner is alive
    st, players, cand = SR.coverage_roots(fog)
    agent = SR.reference_terms(st, None, players, cand, R, depth, SEED, W, H, P, fog=fog)
    assert not np.array_equal(terms, agent)                                  # the rule plays other games than the agent


def test_the_exploration_mix_takes_some_seats_and_leaves_others(monkeypatch):
    taken = {True: 0, False: 0}
    inner = BR.takes_random

    def counted(*a):
        r = bool(inner(*a))
        taken[r] += 1
        return r

    monkeypatch.setattr(BR, "takes_random", counted)
    mixed = _terms(True, 0b11, 500)
    assert taken[True] >= 1 and taken[False] >= 1, taken
    assert 0.3 < taken[True] / (taken[True] + taken[False]) < 0.7, taken    # permille 500 of 6,144 draws
    monkeypatch.setattr(BR, "takes_random", inner)
    assert not np.array_equal(mixed, _terms(True, 0b11, 0))
    assert (mixed[:, :, 0] != mixed[:, :, 1]).any()                          # two replicas of one candidate differ somewhere
