"""The CPU reference of the playout search (tests/_search_reference.py) against its own definition: no GPU.

Roots: 5x5 two-player games after 60 and 100 random-agent turns at mix (0, 0) - old enough that some end inside a playout."""
import numpy as np
import pytest

import _gym_reference as GR
import _oracle as O
import _search_reference as SR

W, H, P = SR.COVER_W, SR.COVER_H, SR.COVER_P
STRIDE = W * H


@pytest.fixture(scope="module", params=[False, True], ids=["nofog", "fog"])
def case(request):
    fog = request.param
    st, players, cand = SR.coverage_roots(fog)
    terms = SR.reference_terms(st, None, players, cand, SR.COVER_R, SR.COVER_D, SR.COVER_SEARCH_SEED, W, H, P, fog=fog, mix=(0, 0))
    return fog, st, players, cand, terms


def test_depth_one_is_one_oracle_step(case):
    """K = R = 1: playout i is env i, so a second batch of the roots themselves, stepped once with the agent's moves and the
    seat's slot replaced, must give the same eight numbers - built here from _gym_reference's decode, not the reference's."""
    fog, st, players, cand, _ = case
    n = len(players)
    one = cand[:, :1]                                                        # every root's first legal move (or padding)
    got = SR.reference_terms(st, None, players, one, 1, 1, 77, W, H, P, fog=fog, mix=(0, 0))[:, 0, 0]
    ora = O.OracleBatch(n, W, H, P, fog=fog)
    ora.set_agent_mix(0, 0)
    ora.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])
    ora.write_state({k: st[k] for k in SR.IMPORTED})
    acts = ora.agent_actions(77)
    playable = (one[:, 0] >= 0) & (st["done"] == 0)
    fx, fy, tx, ty, half, _ = GR.decode_actions(np.where(playable, one[:, 0], 0), W, H)
    for i in np.flatnonzero(playable):
        acts[i, players[i]] = (fx[i], fy[i], tx[i], ty[i], 1, (0, 0, 0))
    ora.step(acts)
    after = ora.read_state()
    assert playable.sum() > 10
    for i in range(n):
        pl, other = int(players[i]), 1 - int(players[i])
        if not playable[i]:
            assert not got[i].any()
            continue
        want = [1, 1, after["alive"][i, pl], int(after["done"][i] and after["winner"][i] == pl), after["tile_count"][i, pl],
                after["army_count"][i, pl], after["tile_count"][i, other], after["army_count"][i, other]]
        assert got[i].tolist() == [int(x) for x in want], i


def test_rows_the_definition_calls_invalid(case):
    fog, st, players, cand, terms = case
    done = st["done"] != 0
    assert done.any() and (~done).any()
    assert not terms[done].any()                                             # a finished root: every row zero
    live = np.flatnonzero(~done & (cand[:, 0] >= 0))
    assert len(live) > 10
    assert (terms[live][:, :4, :, 0] == 1).all()                             # three accepted moves and the half move
    assert not terms[live][:, 4].any()                                       # the index the mask refuses
    assert (terms[live][:, 5, :, 0] == 1).all()                              # the pass is played
    # padding, an index out of range, a seat that is dead, a seat the env does not have, a root outside the batch
    i = int(live[0])
    pl = int(players[i])
    one = lambda a, seat=pl, state=st, env=i: SR.reference_terms(state, [env], [seat], [[a]], 2, 3, 5, W, H, P, fog=fog)[0, 0]
    assert one(int(cand[i, 0]))[:, 0].tolist() == [1, 1]
    for a in (SR.NONE, -3, STRIDE * 5, 2 ** 40):
        assert not one(a).any(), a
    dead = {k: v.copy() for k, v in st.items()}
    dead["alive"][i, pl] = 0
    assert not one(int(cand[i, 0]), state=dead).any() and not one(SR.PASS, state=dead).any()
    assert not one(SR.PASS, seat=P).any() and not one(SR.PASS, seat=-1).any()
    assert not one(SR.PASS, env=len(players)).any() and not one(SR.PASS, env=-1).any()
    assert one(SR.PASS)[:, 0].tolist() == [1, 1]


def test_the_pass_plays_no_move_for_the_seat(case):
    """depth 1, pass: the seat's tiles can only have grown by production or shrunk by the opponent's move - against the
    same playout with the opponent's draw alone (an oracle step where the seat's slot is empty)."""
    fog, st, players, cand, _ = case
    i = int(np.flatnonzero(st["done"] == 0)[0])
    pl = int(players[i])
    got = SR.reference_terms(st, [i], [pl], [[SR.PASS]], 1, 1, 3, W, H, P, fog=fog, mix=(0, 0))[0, 0, 0]
    ora = O.OracleBatch(1, W, H, P, fog=fog)
    ora.set_agent_mix(0, 0)
    one = SR.repeat_state(st, [i])
    ora.reset(one["army"], one["owner"], one["type"], one["width"], one["height"], one["players"])
    ora.write_state({k: one[k] for k in SR.IMPORTED})
    acts = ora.agent_actions(3)
    acts[0, pl] = np.zeros((), O.ACTION_DTYPE)
    ora.step(acts)
    after = ora.read_state()
    assert got[4] == after["tile_count"][0, pl] and got[5] == after["army_count"][0, pl] and got[1] == 1


def test_replicas_differ_and_the_rows_cover_the_rare_outcomes(case):
    """Asserted on the reference alone: among its rows one is won, one ends with the seat dead and one ends early - the
    outcomes the kernel test then has to reproduce."""
    fog, st, players, cand, terms = case
    valid = terms[..., 0] == 1
    assert (terms[:, :, 0] != terms[:, :, 1]).any()                          # two replicas of one candidate differ somewhere
    assert (terms[..., 3] == 1).any(), "no playout is won"
    assert (valid & (terms[..., 2] == 0)).any(), "no playout ends with the seat dead"
    assert (valid & (terms[..., 1] < SR.COVER_D)).any(), "no playout ends before its depth"
    assert (terms[..., 1] <= SR.COVER_D).all() and (terms[valid][:, 1] >= 1).all()
    assert ((terms[..., 3] == 0) | (terms[..., 2] == 1)).all()               # the winner is alive


def test_default_mix_covers_them_too():
    st, players, cand = SR.coverage_roots(True)
    terms = SR.reference_terms(st, None, players, cand, SR.COVER_R, SR.COVER_D, SR.COVER_SEARCH_SEED, W, H, P, fog=True)
    valid = terms[..., 0] == 1
    assert (terms[..., 3] == 1).any() and (valid & (terms[..., 2] == 0)).any() and (valid & (terms[..., 1] < SR.COVER_D)).any()
