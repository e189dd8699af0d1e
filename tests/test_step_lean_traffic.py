"""GPU tests of what the per-turn load path leaves out (DESIGN.md 4.1 "Lean traffic"): the move-target planes rebuilt from
the mountain plane, the dead half of an odd last army slot that is not loaded, and the GEN dwords under the staged plane
store's last chunk - and of what it must keep: ChangedTiles of an env that plays no turn (a frozen one, a gym env whose
action is refused).  Every case runs lock-step against the oracle - full state and packed legal masks after every turn -
through both the per-turn step (gvec_step) and the one-launch gym step (gvec_gym_step)."""
import numpy as np
import pytest

import _harness as H
import _oracle as O
import _state_forms as F

pytestmark = pytest.mark.gpu

B, TURNS, HF_WIDE, MOUNTAIN = 64, 60, 4, 3


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def _boards(seed, sizes, mw, mh, mountains=False):
    """Generated boards; mountains=True walls two of every three free border tiles - every edge, the corners, both ends of
    every row (the row wraps of the flat bit string) - in a pattern that shifts from env to env."""
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, sizes, mw, mh)
    if mountains:
        for e, (w, h, _) in enumerate(sizes):
            for t in range(w * h):
                x, y = t % w, t // w
                border = x in (0, w - 1) or y in (0, h - 1)
                corner = x in (0, w - 1) and y in (0, h - 1)
                if border and typ[e, t] == 0 and owner[e, t] < 0 and (corner or (x + y + e) % 3 != 0):
                    typ[e, t], army[e, t] = MOUNTAIN, 0
        assert all((typ[:, c] == MOUNTAIN).any() for c in (0, sizes[0][0] - 1))
    return army, owner, typ, ws, hs, ps


def _sizes(w, h, P):
    return [(w, h, min(P, max(2, w * h // 30)))] * B  # as many generals as the generator can space out


def _pair(g, boards, mw, mh, P, **kw):
    eng = g.VecEngine(len(boards[0]), mw, mh, P, **kw)
    ora = O.OracleBatch(len(boards[0]), mw, mh, P)
    eng.reset(*boards)
    ora.reset(*boards)
    H.assert_states_equal(eng.game_state(), ora.read_state(), "reset")
    return eng, ora


def _gym_lockstep(g, boards, mw, mh, P, turns=TURNS, ctx="gym"):
    """gvec_gym_step against the oracle: what the kernel will play is read off the same engine first (gvec_agent_actions ->
    gvec_gym_actions, the composition gvec_gym_step is defined as) and handed to the oracle; then the one launch."""
    import torch
    from generalsreinforcementlearning_amd._lib import check
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    n, dev, max_turns = mw * mh, torch.device("cuda"), 25
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    e = g.VecEngine(B, mw, mh, P, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
    ora = O.OracleBatch(B, mw, mh, P)
    e.reset(*boards)
    ora.reset(*boards)
    e.build_board_pool(16, 5)
    ora.set_pool(16, 5)
    turn, obs, mask = z(B, torch.int64), z((B, 9, n), torch.float32), z((B, n * 5), torch.uint8)
    o = {k: z(B, dt) for k, dt in (("reward", torch.float64), ("terminated", torch.uint8), ("truncated", torch.uint8), ("winner", torch.int8),
                                   ("needs_reset", torch.uint8), ("turn_out", torch.int64), ("played", torch.uint8), ("invalid", torch.uint8),
                                   ("error", torch.uint8))}
    resetting, acts_dev = z(B, torch.uint8), z((B, P, 8), torch.uint8)
    check(e.L.gvec_gym_observe(e.h, 0, turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(), None, None, None))
    rng = np.random.default_rng(8)
    refused = kept_changed = 0
    for k in range(turns):
        m = mask.cpu().numpy().astype(bool)
        acts = np.array([rng.choice(np.flatnonzero(r)) if r.any() else 0 for r in m], np.int64)
        if k % 4 == 1:  # refused actions: masked-out indices, out-of-range ones
            acts[:5] = [int(np.flatnonzero(~r)[rng.integers(0, 10)]) for r in m[:5]]
            acts[5], acts[6] = -7, n * 5 + 3
        ta = torch.from_numpy(acts).to(dev)
        seed = 1000 * k + 3
        check(e.L.gvec_agent_actions(e.h, seed, 0, acts_dev.data_ptr(), 1))
        check(e.L.gvec_gym_actions(e.h, 0, ta.data_ptr(), mask.data_ptr(), resetting.data_ptr(), acts_dev.data_ptr(), None, None, None))
        before = e.game_state()
        check(e.L.gvec_gym_step(e.h, 0, seed, ta.data_ptr(), resetting.data_ptr(), turn.data_ptr(), max_turns, obs.data_ptr(), mask.data_ptr(),
                                o["reward"].data_ptr(), o["terminated"].data_ptr(), o["truncated"].data_ptr(), o["winner"].data_ptr(),
                                o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(), o["played"].data_ptr(), o["invalid"].data_ptr(),
                                o["error"].data_ptr()), "gvec_gym_step")
        ora.step(acts_dev.cpu().numpy().reshape(B, P * 8).view(ACTION_DTYPE).reshape(B, P))
        st = e.game_state()
        H.assert_states_equal(st, ora.read_state(), f"{ctx} after turn {k + 1}")
        assert np.array_equal(e.legal_action_mask_bits(), ora.legal_mask()), f"{ctx} turn {k}: legal mask"
        sat_out = np.flatnonzero(o["played"].cpu().numpy() == 0)
        refused += len(sat_out)
        for f in ("changed", "vis_changed", "army"):  # an env whose action was refused keeps every plane, `changed` included
            assert np.array_equal(st[f][sat_out], before[f][sat_out]), (k, f)
        kept_changed += int(before["changed"][sat_out].any(1).sum())  # ... which says something where it was not empty
        resetting.copy_(o["needs_reset"])
    assert refused > 0
    e.kept_changed = kept_changed
    return e, ora


def _both_paths(g, boards, mw, mh, P, seed=3, ctx=""):
    eng, ora = _pair(g, boards, mw, mh, P)
    H.run_lockstep(eng, ora, TURNS, seed=seed, invalid_permille=20, check_every=1, ctx=f"{ctx} step")
    _gym_lockstep(g, boards, mw, mh, P, ctx=f"{ctx} gym")


# ---- A: ok[4] from mtn ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,P", [(5, 7, 2), (8, 8, 2), (16, 4, 2), (20, 20, 4), (13, 32, 4), (32, 32, 8)],
                         ids=["5x7_crosses_a_dword", "8x8_one_slot", "16x4_two_rows_a_dword", "20x20", "13x32", "32x32_p8_full_rows"])
def test_move_targets_on_mountain_boards(g, w, h, P):
    _both_paths(g, _boards(21, _sizes(w, h, P), w, h, mountains=True), w, h, P, ctx=f"{w}x{h}")


def test_move_targets_on_a_mixed_padded_batch(g):
    sizes = [[(10, 10, 2), (15, 15, 3), (20, 20, 4)][i % 3] for i in range(B)]
    _both_paths(g, _boards(22, sizes, 20, 20, mountains=True), 20, 20, 4, ctx="mixed 20x20 handle")


# ---- B: the odd last army slot -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,last_lane", [(20, 20, 15), (13, 32, 31), (21, 20, 35)], ids=["20x20_16_live", "13x32_exactly_32", "21x20_even_lane_35"])
def test_last_army_slot_round_trips(g, w, h, last_lane):
    """The board's last tile - the last live lane of the last slot - is owned with army 50 and moves on the first turn."""
    P, t = 4, w * h - 1
    assert t % 64 == last_lane
    boards = _boards(23, _sizes(w, h, P), w, h)
    army, owner, typ = boards[:3]
    for e in range(B):
        if typ[e, t] != 1:
            typ[e, t], owner[e, t], army[e, t] = 0, 0, 50
        if typ[e, t - w] != 1:
            typ[e, t - w], owner[e, t - w], army[e, t - w] = 0, -1, 0
    eng, ora = _pair(g, boards, w, h, P)
    acts = np.zeros_like(ora.agent_actions(1, 0))  # nobody else moves on this turn
    movers = np.flatnonzero((owner[:, t] == 0) & (typ[:, t] == 0) & (typ[:, t - w] == 0))
    assert len(movers) > B // 2
    for e in movers:
        acts[e, 0] = (w - 1, h - 1, w - 1, h - 2, 1, (0, 0, 0))
    assert np.array_equal(eng.step(acts), ora.step(acts))
    st = eng.game_state()
    H.assert_states_equal(st, ora.read_state(), "after the last tile moved")
    assert (st["army"][movers, t] == 1).all() and (st["army"][movers, t - w] >= 49).all(), (st["army"][movers, t], st["army"][movers, t - w])
    H.run_lockstep(eng, ora, TURNS, seed=5, invalid_permille=20, check_every=1, ctx=f"{w}x{h} step")
    assert (eng.game_state()["army"][:, 64 * (t // 64):].sum(1) > 0).all(), "the last slot is in play in every env"
    _gym_lockstep(g, boards, w, h, P, ctx=f"{w}x{h} gym")


def test_narrow_wide_crossing_with_the_largest_army_on_the_last_slot(g):
    """Tile 399 of a 20x20 board (last slot, lane 15) is player 0's city at 65,534: production carries it over the 16-bit
    boundary, a forced half move brings every army back under it, and it grows over it again."""
    w = h = 20
    P, t = 4, 399
    boards = _boards(24, _sizes(w, h, P), w, h)
    army, owner, typ = boards[:3]
    for e in range(B):
        if typ[e, t] != 1:
            typ[e, t], owner[e, t], army[e, t] = 2, 0, 65534
        if typ[e, t - 1] != 1:
            typ[e, t - 1], owner[e, t - 1], army[e, t - 1] = 0, -1, 0
    ok = np.flatnonzero(typ[:, t] == 2)
    eng, ora = _pair(g, boards, w, h, P)
    saw = []
    for k in range(TURNS):
        acts = ora.agent_actions(9, 20)
        if k % 12 == 8:
            for e in ok:
                acts[e, 0] = (19, 19, 18, 19, 1 | 2, (0, 0, 0))  # half of tile 399 to tile 398
        oerr, obits = ora.step(acts, want_mask=True)
        herr, hbits = eng.step(acts, want_mask=True)
        assert np.array_equal(herr, oerr) and np.array_equal(hbits, obits), k
        st = ora.read_state()
        H.assert_states_equal(eng.game_state(), st, f"turn {k}")
        big = (st["army"].astype(np.int64) > 65535).any(1)
        assert np.array_equal((F.header_flags(eng) & HF_WIDE) != 0, big), k
        saw.append(big[ok].copy())
    saw = np.array(saw)
    crossings = (saw[1:] != saw[:-1]).sum(0)
    assert (crossings >= 2).any(), "some env went narrow -> wide -> narrow"


# ---- C: ChangedTiles of an env that plays no turn (the step kernel loads chg: leaving it out was measured and rejected) --------
def test_frozen_env_keeps_its_changed_tiles(g):
    """auto_reset off, the game over: three more steps (host actions, then the on-device agent) change the header's err
    alone - ChangedTiles, every other plane and the armies stay what the last turn left."""
    w = h = 6
    tiles = [dict(x=0, y=0, owner=0, army=90, type=1), dict(x=1, y=0, owner=1, army=3, type=1), dict(x=5, y=5, owner=0, army=7, type=0),
             dict(x=3, y=3, owner=-1, army=0, type=MOUNTAIN)]
    a, o, t = O.planes_from_tiles(w, h, tiles)
    boards = (np.repeat(a[None], B, 0), np.repeat(o[None], B, 0), np.repeat(t[None], B, 0), [w] * B, [h] * B, [2] * B)
    eng, ora = _pair(g, boards, w, h, 2)
    acts = g.make_actions(B, 2, [(e, 0, 0, 0, 1, 0, True) for e in range(0, B, 2)])  # every other env: general takes general
    assert np.array_equal(eng.step(acts), ora.step(acts))
    before = eng.game_state()
    H.assert_states_equal(before, ora.read_state(), "the capture")
    assert before["done"][::2].all() and not before["done"][1::2].any() and before["changed"][::2].any(1).all()
    for k in range(3):
        acts = ora.agent_actions(4 + k, 20)
        oerr, obits = ora.step(acts, want_mask=True)
        herr, hbits = eng.step(acts, want_mask=True)
        assert np.array_equal(herr, oerr) and (herr[::2] == 5).all() and np.array_equal(hbits, obits)
        st = eng.game_state()
        H.assert_states_equal(st, ora.read_state(), f"frozen step {k}")
        for f in st:
            assert np.array_equal(st[f][::2], before[f][::2]), f
    eng.rollout(3, seed=2, fused=False)  # the on-device agent's variant of the step kernel
    st = eng.game_state()
    for f in st:
        assert np.array_equal(st[f][::2], before[f][::2]), f


def test_refused_gym_env_keeps_its_changed_tiles(g):
    """A gym env whose action is refused plays no turn: its ChangedTiles - not empty - are what the last turn left
    (_gym_lockstep compares every refused env's planes with the state before the call)."""
    w = h = 20
    e, _ = _gym_lockstep(g, _boards(26, _sizes(w, h, 4), w, h), w, h, 4, turns=24, ctx="refused gym")
    assert e.kept_changed > 0, "no refused env had a tile in ChangedTiles: the comparison above said nothing"


# ---- D: the GEN dwords under the folded chunk --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,P,rem", [(9, 10, 4, 1), (8, 8, 4, 2), (20, 20, 4, 3), (21, 20, 4, 2), (5, 5, 2, 3), (14, 15, 2, 1)],
                         ids=["9x10_p4_rem1", "8x8_p4_rem2", "20x20_p4_rem3", "21x20_p4_rem2", "5x5_p2_rem3", "14x15_p2_rem1"])
def test_general_positions_survive_the_folded_chunk(g, w, h, P, rem):
    fd = -(-w * h // 32)
    assert ((2 * P + 3) * fd) % 4 == rem and 4 - rem <= fd
    boards = _boards(25, _sizes(w, h, P), w, h)
    typ0 = boards[2].copy()
    assert (typ0[:, :32 * (4 - rem)] == 1).any(), "a general sits under the folded dwords"
    eng, ora = _pair(g, boards, w, h, P)
    H.run_lockstep(eng, ora, TURNS, seed=6, invalid_permille=20, check_every=1, ctx=f"{w}x{h} step")
    assert np.array_equal(eng.game_state()["type"], typ0)
    e, ora = _gym_lockstep(g, boards, w, h, P, turns=20, ctx=f"{w}x{h} gym")
    assert np.array_equal(e.game_state()["type"] == 1, ora.read_state()["type"] == 1)
