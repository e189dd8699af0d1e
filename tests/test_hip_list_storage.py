"""GPU tests of the on-demand OwnedTiles planes (gvec_device.hpp HF_LDIFF): a player's list is stored separately from
the ownership planes only while the two differ - after an aborted turn, until a stats pass heals it.
The flagged envs must survive every way state moves (step, fused rollout, record slabs, write_state pokes) exactly
like the unflagged ones; expected values come from the oracle, which keeps the reference's explicit lists."""
import numpy as np
import pytest

import _harness as H
import _state_forms as F
import _oracle as O

pytestmark = pytest.mark.gpu

HF_LDIFF = 128


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def _desynced(st):
    """envs in which some tile is owned by a player that does not list it (or listed by one that does not own it)"""
    return np.flatnonzero((st["listed"] != st["owner"]).any(axis=1))


def _make_desynced(g, B, w, h, P, seed):
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, [(w, h, P)] * B, w, h)
    eng, ora = g.VecEngine(B, w, h, P), O.OracleBatch(B, w, h, P)
    eng.reset(army, owner, typ, ws, hs, ps)
    ora.reset(army, owner, typ, ws, hs, ps)
    H.run_lockstep(eng, ora, 60, seed, invalid_permille=80, check_every=5, ctx="warm-up with invalid moves")
    return eng, ora


@pytest.mark.parametrize("w,h,P", [(10, 10, 2), (20, 20, 4), (32, 32, 8)], ids=["10x10_p2", "20x20_p4", "32x32_p8"])
def test_flag_is_set_exactly_where_lists_differ_from_ownership(g, w, h, P):
    eng, ora = _make_desynced(g, 128, w, h, P, 21)
    seen = 0
    for k in range(40):
        acts = ora.agent_actions(21, 80)
        ora.step(acts)
        eng.step(acts)
        st = eng.game_state()
        H.assert_states_equal(st, ora.read_state(), f"turn {k}")
        want = np.zeros(eng.B, bool)
        want[_desynced(st)] = True
        assert np.array_equal((F.header_flags(eng) & HF_LDIFF) != 0, want), f"turn {k}: HF_LDIFF <=> listed != owner"
        seen += int(want.sum())
    assert seen > 20, "the scenario must actually produce envs whose lists differ (aborted turns, H5/H6)"


def test_desynced_envs_travel_in_record_slabs_and_play_on(g):
    import torch
    B, w, h, P = 96, 20, 20, 4
    a, ora = _make_desynced(g, B, w, h, P, 33)
    st = a.game_state()
    assert len(_desynced(st)) > 0
    b = g.VecEngine(B, w, h, P)
    buf = torch.zeros(B * a.state_bytes_per_env(), dtype=torch.uint8, device="cuda")
    a.export_records(buf.data_ptr())
    a.synchronize()
    b.import_records(buf.data_ptr())
    sb = b.game_state()
    for f in st:
        assert np.array_equal(st[f], sb[f]), f
    assert np.array_equal(F.header_flags(a) & HF_LDIFF, F.header_flags(b) & HF_LDIFF)
    # both copies keep following the oracle, through turns that heal some lists and break others
    for k in range(30):
        acts = ora.agent_actions(33, 80)
        oerr = ora.step(acts)
        assert np.array_equal(a.step(acts), oerr) and np.array_equal(b.step(acts), oerr), f"turn {k}"
        if k % 5 == 4:
            H.assert_states_equal(a.game_state(), ora.read_state(), f"exporter, turn {k}")
            H.assert_states_equal(b.game_state(), ora.read_state(), f"importer, turn {k}")


def test_write_state_pokes_of_the_lists_are_kept_and_healed_like_the_reference(g):
    """The Go tests assign e.gs.* directly; a poked list must read back as written, set the flag, and be treated by the
    next stats pass exactly as the oracle treats it (stats.go:90-130: dropped where not owned, re-added only via C)."""
    B, w, h, P = 16, 12, 12, 3
    army, owner, typ, ws, hs, ps = H.gen_boards(4, [(w, h, P)] * B, w, h)
    eng, ora = g.VecEngine(B, w, h, P), O.OracleBatch(B, w, h, P)
    eng.reset(army, owner, typ, ws, hs, ps)
    ora.reset(army, owner, typ, ws, hs, ps)
    H.run_lockstep(eng, ora, 12, 4, check_every=4, ctx="warm-up")
    st = ora.read_state()
    listed = st["listed"].copy()
    rng = np.random.default_rng(9)
    for e in range(0, B, 2):                                   # every other env: unlist a few owned, non-general tiles
        mine = np.flatnonzero((st["owner"][e] >= 0) & (st["type"][e] != 1))
        listed[e, rng.choice(mine, size=min(3, len(mine)), replace=False)] = -1
    eng.write_state({"listed": listed})
    ora.write_state({"listed": listed})
    got = eng.game_state()
    assert np.array_equal(got["listed"], listed)
    want = np.zeros(B, bool)
    want[_desynced(got)] = True
    assert want[::2].all() and not want[1::2].any()
    assert np.array_equal((F.header_flags(eng) & HF_LDIFF) != 0, want)
    H.run_lockstep(eng, ora, 40, 5, invalid_permille=30, check_every=1, ctx="after the poke")


def test_fused_rollout_carries_flagged_envs(g):
    """The K-turn kernel loads the lists by the flag and settles it at its one store."""
    B, w, h, P = 128, 15, 15, 2
    eng, ora = _make_desynced(g, B, w, h, P, 55)
    assert len(_desynced(eng.game_state())) > 0
    eng.rollout(25, seed=8, invalid_permille=60, fused=True)
    ora.rollout(25, 8, 60)
    st = eng.game_state()
    H.assert_states_equal(st, ora.read_state(), "after 25 fused turns")
    want = np.zeros(B, bool)
    want[_desynced(st)] = True
    assert np.array_equal((F.header_flags(eng) & HF_LDIFF) != 0, want)
