"""Self-play: gvec_gym_observe_players / gvec_gym_step_players (every learner of a player set in one launch) and
GeneralsSelfPlayVecEnv on top of them.  Checked against (a) the existing single-learner composition, adjusted to the
refusal rule of the new call (a refused action is no move; the env still plays), (b) the numpy restatement of the gym
env (tests/_gym_reference.py) per learner and the CPU oracle for the turn, (c) a twin engine driven by gvec_agent_actions
+ gvec_step for a mixed table of learners and agents."""
import ctypes as C

import numpy as np
import pytest

import _gym_reference as G
import _harness as H
import _oracle as O

B = 64
DIRS = ((0, -1), (1, 0), (0, 1), (-1, 0))
LAYOUTS = [(9, 8, 2, True), (20, 20, 4, True), (12, 13, 3, False), (25, 25, 4, True), (32, 32, 8, True), (5, 5, 2, True), (16, 16, 2, True),
           (21, 21, 8, True), (25, 24, 8, False), (30, 32, 2, True), (11, 11, 4, True)]
LAYOUT_IDS = ["9x8_p2", "20x20_p4", "12x13_p3_nofog", "25x25_p4", "32x32_p8", "5x5_p2", "16x16_p2", "21x21_p8", "25x24_p8_nofog",
              "30x32_p2", "11x11_p4"]
OUTS = ("reward", "invalid", "error", "alive", "terminated", "truncated", "winner", "needs_reset", "turn_out")


def _z(shape, dt):
    import torch
    return torch.zeros(shape, dtype=dt, device="cuda")


class Players:
    """One handle driven by gvec_gym_step_players for the learners of bit set `bits`."""

    def __init__(self, w, h, P, fog, bits, max_turns, pool=16, production=(1, 1, 1), normal_growth_interval=25):
        import torch
        import generalsreinforcementlearning_amd as g
        from generalsreinforcementlearning_amd._lib import check
        self.check, self.w, self.h, self.P, self.bits, self.max_turns = check, w, h, P, bits, max_turns
        self.ids = [p for p in range(P) if (bits >> p) & 1]
        L, n = len(self.ids), w * h
        self.e = g.VecEngine(B, w, h, P, fog_of_war=fog, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream,
                             production=production, normal_growth_interval=normal_growth_interval)
        self.e.reset_generated(77)
        self.e.build_board_pool(pool, 5)
        self.turn, self.resetting = _z(B, torch.int64), _z(B, torch.uint8)
        self.obs, self.mask = _z((B, L, 9, n), torch.float32), _z((B, L, n * 5), torch.uint8)
        self.out = {"reward": _z((B, L), torch.float64), "invalid": _z((B, L), torch.uint8), "error": _z((B, L), torch.uint8),
                    "alive": _z((B, L), torch.uint8), "terminated": _z(B, torch.uint8), "truncated": _z(B, torch.uint8),
                    "winner": _z(B, torch.int8), "needs_reset": _z(B, torch.uint8), "turn_out": _z(B, torch.int64)}
        self.done0 = _z(B, torch.uint8)
        e = self.e
        check(e.L.gvec_gym_observe_players(e.h, bits, self.turn.data_ptr(), max_turns, self.obs.data_ptr(), self.mask.data_ptr(),
                                           self.out["reward"].data_ptr(), self.done0.data_ptr(), self.out["winner"].data_ptr()),
              "gvec_gym_observe_players")

    def step(self, acts, seed):
        import torch
        ta = torch.from_numpy(np.ascontiguousarray(acts, np.int64).reshape(B, len(self.ids))).cuda()
        e, o = self.e, self.out
        self.check(e.L.gvec_gym_step_players(e.h, self.bits, seed, ta.data_ptr(), self.resetting.data_ptr(), self.turn.data_ptr(), self.max_turns,
                                             self.obs.data_ptr(), self.mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(),
                                             o["truncated"].data_ptr(), o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(),
                                             o["invalid"].data_ptr(), o["error"].data_ptr(), o["alive"].data_ptr()), "gvec_gym_step_players")
        return self.outputs()

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy().copy() for k, v in self.out.items()}
        d["obs"], d["mask"], d["turn"] = self.obs.cpu().numpy().view(np.uint32).copy(), self.mask.cpu().numpy().copy(), self.turn.cpu().numpy().copy()
        return d

    def next_step(self):
        self.resetting.copy_(self.out["needs_reset"])


class Composed:
    """gvec_agent_actions -> gvec_gym_actions(p) -> gvec_step -> gvec_gym_finish_step(p) with the self-play refusal rule:
    a refused action is no move but the env plays (GVEC_ACT_SKIP_ENV cleared, played = 1), it costs -0.1 when the
    learner was alive, and a learner that was not alive keeps invalid / error 0."""

    def __init__(self, w, h, P, fog, p, max_turns, pool=16):
        import torch
        import generalsreinforcementlearning_amd as g
        from generalsreinforcementlearning_amd._lib import check
        self.check, self.p, self.P, self.max_turns = check, p, P, max_turns
        n = w * h
        self.e = g.VecEngine(B, w, h, P, fog_of_war=fog, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
        self.e.reset_generated(77)
        self.e.build_board_pool(pool, 5)
        self.turn, self.resetting = _z(B, torch.int64), _z(B, torch.uint8)
        self.obs, self.mask = _z((B, 9, n), torch.float32), _z((B, n * 5), torch.uint8)
        self.acts, self.played = _z((B, P, 8), torch.uint8), _z(B, torch.uint8)
        self.out = {k: _z(B, dt) for k, dt in (("reward", torch.float64), ("terminated", torch.uint8), ("truncated", torch.uint8),
                                              ("winner", torch.int8), ("needs_reset", torch.uint8), ("turn_out", torch.int64),
                                              ("invalid", torch.uint8), ("error", torch.uint8))}
        self.done0 = _z(B, torch.uint8)
        e = self.e
        check(e.L.gvec_gym_observe(e.h, p, self.turn.data_ptr(), max_turns, self.obs.data_ptr(), self.mask.data_ptr(),
                                   self.out["reward"].data_ptr(), self.done0.data_ptr(), self.out["winner"].data_ptr()))

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy().copy() for k, v in self.out.items()}
        d["obs"], d["mask"], d["turn"] = self.obs.cpu().numpy().view(np.uint32).copy(), self.mask.cpu().numpy().copy(), self.turn.cpu().numpy().copy()
        return d

    def step(self, acts, seed):
        import torch
        st = self.e.game_state(fields=("alive", "players"))
        counted = (st["alive"][:, self.p] != 0) & (self.p < st["players"])
        ta = torch.from_numpy(np.ascontiguousarray(acts, np.int64).reshape(B)).cuda()
        e, o, L, p = self.e, self.out, self.e.L, self.p
        prev_mask = self.mask.clone()
        self.check(L.gvec_agent_actions(e.h, seed, 0, self.acts.data_ptr(), 1))
        self.check(L.gvec_gym_actions(e.h, p, ta.data_ptr(), prev_mask.data_ptr(), self.resetting.data_ptr(), self.acts.data_ptr(),
                                      self.played.data_ptr(), o["invalid"].data_ptr(), o["error"].data_ptr()))
        self.acts[:, 0, 4] &= 0xFB                # GVEC_ACT_SKIP_ENV off: the env plays its turn
        self.played.fill_(1)
        e.step_device(self.acts.data_ptr())
        self.check(L.gvec_gym_finish_step(e.h, p, self.turn.data_ptr(), self.max_turns, self.resetting.data_ptr(), self.played.data_ptr(),
                                          self.obs.data_ptr(), self.mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(),
                                          o["truncated"].data_ptr(), o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr()))
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy().copy() for k, v in o.items()}
        refused = (d["invalid"] | d["error"]).astype(bool) & counted
        d["reward"] = np.where(refused, d["reward"] - 0.1, d["reward"])
        d["invalid"] = d["invalid"] & counted
        d["error"] = d["error"] & counted
        d["alive"] = self.e.game_state(fields=("alive",))["alive"][:, p].copy()
        d["obs"], d["mask"], d["turn"] = self.obs.cpu().numpy().view(np.uint32).copy(), self.mask.cpu().numpy().copy(), self.turn.cpu().numpy().copy()
        return d

    def next_step(self):
        self.resetting.copy_(self.out["needs_reset"])


def _mixed_actions(rng, mask, k, n):
    """test_gym_step_equals_the_four_call_composition's action mix: valid, masked-off, out-of-range and half moves."""
    acts = np.array([rng.choice(np.flatnonzero(m)) if m.any() else 0 for m in mask], np.int64)
    if k % 4 == 1:
        acts[:5] = [int(np.flatnonzero(~m)[rng.integers(0, 10)]) for m in mask[:5]]
        acts[5], acts[6] = -7, n * 5 + 3
    if k % 3 == 0:
        for e_ in range(8, 24):
            hm = np.flatnonzero(mask[e_][4::5])
            if len(hm):
                acts[e_] = int(hm[rng.integers(0, len(hm))]) * 5 + 4
    return acts


def _assert_same(a, b, k, names):
    for f in names:
        x, y = np.asarray(a[f]).reshape(B, -1), np.asarray(b[f]).reshape(B, -1)
        if f == "reward":
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), (k, f, np.flatnonzero((x != y).any(1))[:8])


# ---- 1. one learner == the adjusted single-learner composition ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("last", [False, True], ids=["p0", "plast"])
@pytest.mark.parametrize("w,h,P,fog", LAYOUTS, ids=LAYOUT_IDS)
def test_one_learner_equals_the_adjusted_composition(w, h, P, fog, last):
    p, max_turns, n = (P - 1 if last else 0), 25, w * h
    one, four = Players(w, h, P, fog, 1 << p, max_turns), Composed(w, h, P, fog, p, max_turns)
    a, b = one.outputs(), four.outputs()
    _assert_same(a, b, -1, ("obs", "mask", "reward", "winner"))
    rng = np.random.default_rng(8 + p)
    seen = {"trunc": 0, "invalid": 0, "error": 0, "reset": 0, "refused_played": 0}
    for k in range(120):
        mask = one.mask.cpu().numpy()[:, 0].astype(bool)
        acts = _mixed_actions(rng, mask, k, n)
        seed = 1000 * k + 3
        resetting = one.resetting.cpu().numpy().astype(bool)
        a, b = one.step(acts[:, None], seed), four.step(acts, seed)
        _assert_same(a, b, k, OUTS + ("obs", "mask", "turn"))
        seen["trunc"] += int(a["truncated"].sum()); seen["reset"] += int(resetting.sum())
        seen["invalid"] += int(a["invalid"].sum()); seen["error"] += int(a["error"].sum())
        seen["refused_played"] += int(((a["invalid"] | a["error"])[:, 0].astype(bool) & (a["turn"] > 0)).sum())
        one.next_step(); four.next_step()
    assert seen["trunc"] > 0 and seen["invalid"] > 0 and seen["reset"] > 0 and seen["refused_played"] > 0, seen
    H.assert_states_equal(one.e.game_state(), four.e.game_state(), "step_players vs adjusted composition")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog,p", [(9, 8, 2, True, 1), (20, 20, 4, True, 0), (12, 13, 3, False, 2), (32, 32, 8, True, 7)],
                         ids=["9x8_p2_pl1", "20x20_p4_pl0", "12x13_p3_nofog_pl2", "32x32_p8_pl7"])
def test_one_learner_with_accepted_moves_equals_gym_step(w, h, P, fog, p):
    """While every action is accepted the new call IS gvec_gym_step(p): outputs and states bit for bit."""
    import torch
    max_turns = 500
    one = Players(w, h, P, fog, 1 << p, max_turns)
    e2 = Composed(w, h, P, fog, p, max_turns)          # only its handle, turn counter and buffers: driven by gvec_gym_step
    e, o = e2.e, e2.out
    played = _z(B, torch.uint8)
    rng = np.random.default_rng(3)
    steps = 0
    for k in range(40):
        mask = one.mask.cpu().numpy()[:, 0].astype(bool)
        full = mask.reshape(B, -1, 5)[:, :, :4].reshape(B, -1)
        if not full.any(1).all():
            break
        acts = np.array([(lambda i: (i // 4) * 5 + i % 4)(int(rng.choice(np.flatnonzero(m)))) for m in full], np.int64)
        seed = 77 * k + 1
        a = one.step(acts[:, None], seed)
        ta = torch.from_numpy(acts).cuda()
        e2.check(e.L.gvec_gym_step(e.h, p, seed, ta.data_ptr(), e2.resetting.data_ptr(), e2.turn.data_ptr(), max_turns, e2.obs.data_ptr(),
                                   e2.mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(), o["truncated"].data_ptr(),
                                   o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(), played.data_ptr(),
                                   o["invalid"].data_ptr(), o["error"].data_ptr()), "gvec_gym_step")
        torch.cuda.synchronize()
        b = {f: v.cpu().numpy() for f, v in o.items()}
        b["obs"], b["mask"], b["turn"] = e2.obs.cpu().numpy().view(np.uint32), e2.mask.cpu().numpy(), e2.turn.cpu().numpy()
        assert played.cpu().numpy().all() and not a["invalid"].any() and not a["error"].any()
        _assert_same(a, b, k, ("reward", "invalid", "error", "terminated", "truncated", "winner", "needs_reset", "turn_out", "obs", "mask", "turn"))
        one.next_step(); e2.next_step()
        steps += 1
    assert steps >= 5, steps
    H.assert_states_equal(one.e.game_state(), e.game_state(), "step_players vs gym_step")


# ---- 2. every player a learner: the restatement per learner, the oracle for the turn ---------------------------------
def _stats(st):
    return {k: st[k].copy() for k in ("done", "winner", "alive", "army_count", "tile_count")}


def _plant_capture(eng, envs, w, h, q):
    """Player 0 takes player q's general with its next move: a 1000-army tile of player 0 next to the general, which holds 1.
    Returns {env: player 0's action index}."""
    st = eng.game_state()
    moves = {}
    for e in envs:
        g = int(st["general_idx"][e, q])
        if g < 0 or not st["alive"][e, 0] or not st["alive"][e, q]:
            continue
        gx, gy = g % w, g // w
        for d, (dx, dy) in enumerate(DIRS):
            tx, ty = gx - dx, gy - dy
            t = ty * w + tx
            if not (0 <= tx < w and 0 <= ty < h) or st["type"][e, t] != 0:
                continue
            st["owner"][e, t], st["listed"][e, t], st["army"][e, t], st["army"][e, g] = 0, 0, 1000, 1
            st["visible"][e, t] |= 1
            st["visible"][e, g] |= 1
            moves[e] = t * 5 + d
            break
    eng.write_state({k: st[k] for k in ("owner", "listed", "army", "visible")})
    return moves


def _expected_decode(acts, masks0, ids, w, h, st0, rs):
    """Per learner (column j): valid, accepted, half, decoded move, and whether its flags / penalty count."""
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    n5 = w * h * 5
    res = []
    for j, p in enumerate(ids):
        a = acts[:, j]
        in_range = (a >= 0) & (a < n5)
        ac = np.where(in_range, a, 0)
        valid = in_range & masks0[j][np.arange(B), ac]
        fx, fy, tx, ty, half, d = G.decode_actions(ac, w, h)
        accepted = valid & masks0[j][np.arange(B), (fy * w + fx) * 5 + d]
        counted = ~rs & (st0["alive"][:, p] != 0) & (p < st0["players"])
        res.append(dict(valid=valid, accepted=accepted, half=half, counted=counted, in_range=in_range, move=(fx, fy, tx, ty)))
    return res


def _check_learners(out, eng, ids, dec, prev, rs, turn_exp, w, h, max_turns, ctx):
    """Every learner's observation / mask / reward / flags and the env flags against the restatement of the new state."""
    st1 = eng.game_state()
    cur = _stats(st1)
    n = w * h
    for j, p in enumerate(ids):
        vis, fog = eng.compute_player_visibility(p)
        view = G.proto_view(st1["owner"], st1["army"], st1["type"], vis, fog)
        obs = G.build_observation(view, p, turn_exp, max_turns, w, h).reshape(B, 9 * n)
        assert np.array_equal(out["obs"][:, j].reshape(B, -1), obs.view(np.uint32)), (ctx, p, "obs")
        assert np.array_equal(out["mask"][:, j].astype(bool), G.valid_actions_mask(view, p, w, h)), (ctx, p, "mask")
        r = G.calculate_reward(prev, cur, p)
        d = dec[j]
        r = np.where(rs, 0.0, np.where(d["counted"] & ~d["accepted"], r - 0.1, r))
        assert np.array_equal(out["reward"][:, j].view(np.uint64), r.view(np.uint64)), (ctx, p, "reward", np.flatnonzero(out["reward"][:, j] != r)[:8])
        assert np.array_equal(out["invalid"][:, j].astype(bool), ~d["valid"] & d["counted"]), (ctx, p, "invalid")
        assert np.array_equal(out["error"][:, j].astype(bool), d["valid"] & ~d["accepted"] & d["counted"]), (ctx, p, "error")
        assert np.array_equal(out["alive"][:, j], st1["alive"][:, p]), (ctx, p, "alive")
    term = st1["done"].astype(bool) & ~rs
    trunc = (turn_exp >= max_turns) & ~rs
    assert np.array_equal(out["turn"], turn_exp) and np.array_equal(out["turn_out"], turn_exp), ctx
    assert np.array_equal(out["terminated"].astype(bool), term) and np.array_equal(out["truncated"].astype(bool), trunc), ctx
    assert np.array_equal(out["needs_reset"].astype(bool), term | trunc), ctx
    assert np.array_equal(out["winner"], np.where(term, st1["winner"], -1)), ctx
    return st1, cur


def _learner_actions(rng, masks0, k, n, L, w, h):
    acts = np.stack([_mixed_actions(rng, masks0[j], k + j, n) for j in range(L)], 1)
    for e_ in range(24, 30):                         # half moves the first-direction rule turns into a refused move
        j = e_ % L
        m = masks0[j][e_]
        cand = np.flatnonzero(m[4::5])
        if len(cand):
            fx, fy, _, _, _, d = G.decode_actions(cand * 5 + 4, w, h)
            bad = cand[~m[cand * 5 + d]]
            if len(bad):
                acts[e_, j] = int(bad[rng.integers(0, len(bad))]) * 5 + 4
    if k % 5 == 2:                                   # one learner refused, the others valid: the env still plays
        for e_ in range(40, 48):
            acts[e_, e_ % L] = -1
    return acts


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog", [(10, 10, 2, True), (15, 15, 2, True), (21, 13, 3, True), (20, 20, 4, True), (25, 25, 4, True),
                                       (32, 32, 8, True), (12, 12, 3, False)],
                         ids=["10x10_p2", "15x15_p2", "21x13_p3", "20x20_p4", "25x25_p4", "32x32_p8", "12x12_p3_nofog"])
def test_every_player_a_learner_matches_restatement_and_oracle(w, h, P, fog):
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    max_turns, n = 20, w * h
    sp = Players(w, h, P, fog, (1 << P) - 1, max_turns)
    ids, L = sp.ids, len(sp.ids)
    eng = sp.e
    ora = O.OracleBatch(B, w, h, P, fog=fog)
    st = eng.game_state()
    ora.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])   # the envs write_state fills
    rng = np.random.default_rng(11)
    prev = _stats(eng.game_state())
    seen = dict(out_of_range=0, masked=0, half_refused=0, mixed=0, term=0, trunc=0, reset=0, eliminated_learner=0)
    turn = np.zeros(B, np.int64)
    for k in range(45):
        # player 0 eliminates players 1 .. P-1 of envs 30-33 one after the other (twice: the second time after the re-deal)
        q = [q_ for q_ in range(1, P) if k in (4 + 2 * (q_ - 1), 26 + 2 * (q_ - 1))]
        planted = _plant_capture(eng, range(30, 34), w, h, q[0]) if q else {}
        st0 = eng.game_state()
        rs = sp.resetting.cpu().numpy().astype(bool)
        masks0 = []
        for p in ids:
            vis, fog_ = eng.compute_player_visibility(p)
            masks0.append(G.valid_actions_mask(G.proto_view(st0["owner"], st0["army"], st0["type"], vis, fog_), p, w, h))
        acts = _learner_actions(rng, masks0, k, n, L, w, h)
        for e_, a in planted.items():
            acts[e_, 0] = a
        dec = _expected_decode(acts, masks0, ids, w, h, st0, rs)
        out = sp.step(acts, 500 + k)
        turn = np.where(rs, 0, turn + 1)
        st1, cur = _check_learners(out, eng, ids, dec, prev, rs, turn, w, h, max_turns, f"{w}x{h} step {k}")
        # the turn: the oracle from the pre-step state, with the accepted learner moves (a refused learner: no move)
        oacts = np.zeros((B, P), ACTION_DTYPE)
        for j, p in enumerate(ids):
            fx, fy, tx, ty = dec[j]["move"]
            acc = dec[j]["accepted"]
            oacts["from_x"][:, p], oacts["from_y"][:, p] = np.where(acc, fx, 0), np.where(acc, fy, 0)
            oacts["to_x"][:, p], oacts["to_y"][:, p] = np.where(acc, tx, 0), np.where(acc, ty, 0)
            oacts["flags"][:, p] = np.where(acc, G.ACT_VALID | np.where(dec[j]["half"], G.ACT_HALF, 0), 0)
        ora.write_state(st0)
        ora.step(oacts)
        keep = ~rs & ~st0["done"].astype(bool)
        ost = ora.read_state()
        H.assert_states_equal({f: v[keep] for f, v in st1.items()}, {f: v[keep] for f, v in ost.items()}, f"{w}x{h} step {k} vs oracle")
        for j, p in enumerate(ids):
            d = dec[j]
            inv = ~d["valid"] & d["counted"]
            seen["out_of_range"] += int((inv & ~d["in_range"]).sum())
            seen["masked"] += int((inv & d["in_range"]).sum())
            seen["half_refused"] += int((d["valid"] & ~d["accepted"] & d["half"] & d["counted"]).sum())
            seen["eliminated_learner"] += int((~rs & (st0["alive"][:, p] == 0) & (p < st0["players"])).sum())
        refused = np.stack([d["counted"] & ~d["accepted"] for d in dec], 1)
        accepted = np.stack([d["counted"] & d["accepted"] for d in dec], 1)
        seen["mixed"] += int((refused.any(1) & accepted.any(1)).sum())
        seen["term"] += int(out["terminated"].sum()); seen["trunc"] += int(out["truncated"].sum()); seen["reset"] += int(rs.sum())
        prev = cur
        sp.next_step()
    assert all(v > 0 for k_, v in seen.items() if k_ != "eliminated_learner"), seen
    if P > 2:
        assert seen["eliminated_learner"] > 0, seen


# ---- 3. a mixed table: learners {0, 2} of four players ----------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_table_equals_agent_twin_with_learner_slots():
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    w, h, P, max_turns, n = 14, 15, 4, 20, 14 * 15
    sp = Players(w, h, P, True, 0b101, max_turns)
    twin = g.VecEngine(B, w, h, P, auto_reset=True)
    twin.reset_generated(77)
    twin.build_board_pool(16, 5)
    ids, eng = sp.ids, sp.e
    rng = np.random.default_rng(5)
    prev = _stats(eng.game_state())
    turn = np.zeros(B, np.int64)
    refused_total = 0
    for k in range(50):
        st0 = eng.game_state()
        rs = sp.resetting.cpu().numpy().astype(bool)
        masks0 = []
        for p in ids:
            vis, fog = eng.compute_player_visibility(p)
            masks0.append(G.valid_actions_mask(G.proto_view(st0["owner"], st0["army"], st0["type"], vis, fog), p, w, h))
        acts = _learner_actions(rng, masks0, k, n, 2, w, h)
        dec = _expected_decode(acts, masks0, ids, w, h, st0, rs)
        seed = 900 + 7 * k
        out = sp.step(acts, seed)
        turn = np.where(rs, 0, turn + 1)
        st1, cur = _check_learners(out, eng, ids, dec, prev, rs, turn, w, h, max_turns, f"mixed step {k}")
        ta = twin.agent_actions(seed, 0)
        for j, p in enumerate(ids):
            fx, fy, tx, ty = dec[j]["move"]
            acc = dec[j]["accepted"]
            ta["from_x"][:, p], ta["from_y"][:, p], ta["to_x"][:, p], ta["to_y"][:, p] = fx, fy, tx, ty
            ta["flags"][:, p] = np.where(acc, G.ACT_VALID | np.where(dec[j]["half"], G.ACT_HALF, 0), 0)
        ta["flags"][:, 0] = np.where(rs, ta["flags"][:, 0] | G.ACT_RESET_ENV, ta["flags"][:, 0])
        twin.step(ta)
        H.assert_states_equal(st1, twin.game_state(), f"mixed table step {k}")
        refused_total += int(sum((d["counted"] & ~d["accepted"]).sum() for d in dec))
        prev = cur
        sp.next_step()
    assert refused_total > 0


# ---- 4. the second side's reward -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_second_player_reward_is_shaped():
    """2P self-play: player 1's reward is _calculate_reward(prev, cur, 1) - nonzero and non-terminal on some steps (the
    single-learner composition measures the second side against stats the first side's call has just refreshed)."""
    w, h, max_turns = 15, 15, 500
    sp = Players(w, h, 2, True, 0b11, max_turns)
    eng = sp.e
    rng = np.random.default_rng(2)
    prev = _stats(eng.game_state())
    shaped = 0
    for k in range(30):
        mask = sp.mask.cpu().numpy().astype(bool)
        acts = np.stack([[rng.choice(np.flatnonzero(m)) if m.any() else 0 for m in mask[:, j]] for j in range(2)], 1).astype(np.int64)
        out = sp.step(acts, 31 + k)
        cur = _stats(eng.game_state())
        r1 = G.calculate_reward(prev, cur, 1)
        r1 = np.where(out["invalid"][:, 1] | out["error"][:, 1], r1 - 0.1, r1)
        assert np.array_equal(out["reward"][:, 1].view(np.uint64), r1.view(np.uint64)), k
        shaped += int(((r1 != 0) & (np.abs(r1) != 100) & ~cur["done"].astype(bool)).sum())
        prev = cur
        sp.next_step()
    assert shaped > 0


# ---- 5. the Python env --------------------------------------------------------------------------------------------------
def _policy(rng, mask):
    return np.array([[rng.choice(np.flatnonzero(m)) if m.any() else 0 for m in row] for row in mask], np.int64)


@pytest.mark.gpu
def test_selfplay_env_shapes_modes_buffers_and_force_reset():
    import torch
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    kw = dict(board_width=9, board_height=8, max_players=3, learners=[2, 0], max_turns=15, seed=6, board_pool=16)
    a = GeneralsSelfPlayVecEnv(B, device_outputs=False, **kw)
    d = GeneralsSelfPlayVecEnv(B, device_outputs=True, **kw)
    assert a.player_ids == [0, 2] and a.num_learners == 2
    oa, ia = a.reset()
    od, idd = d.reset()
    assert oa.shape == (B, 2, 9, 8, 9) and oa.dtype == np.float32 and ia["valid_actions_mask"].shape == (B, 2, 9 * 8 * 5)
    assert ia["valid_actions_mask"].dtype == bool and ia["player_ids"] == [0, 2] and ia["turn"].shape == (B,)
    assert isinstance(od, torch.Tensor) and od.is_cuda and np.array_equal(oa, od.cpu().numpy())
    rng = np.random.default_rng(0)
    prev_dev = None
    for k in range(30):
        acts = _policy(rng, ia["valid_actions_mask"])
        if k == 10:
            a.force_reset(np.arange(B) < 8)
            d.force_reset(torch.arange(B, device="cuda") < 8)
        ra = a.step(acts)
        rd = d.step(torch.from_numpy(acts).cuda())
        obs, reward, term, trunc, info = ra
        assert obs.shape == (B, 2, 9, 8, 9) and reward.shape == (B, 2) and reward.dtype == np.float64
        assert term.shape == (B,) and trunc.shape == (B,) and term.dtype == bool
        for f in ("invalid", "error", "alive"):
            assert info[f].shape == (B, 2) and info[f].dtype == bool, f
        assert set(info) == {"turn", "valid_actions_mask", "invalid", "error", "alive", "winner", "reset"}
        for x, y in zip(ra[:4], rd[:4]):
            assert np.array_equal(x, y.cpu().numpy()), k
        for f in info:
            assert np.array_equal(info[f], rd[4][f].cpu().numpy()), (k, f)
        if k == 10:
            assert info["reset"][:8].all() and (info["turn"][:8] == 0).all()
        # the reuse rule: what step k returned is intact after step k + 1 and overwritten by step k + 2
        if prev_dev is not None:
            snap, ref = prev_dev
            assert torch.equal(snap, ref), k
        prev_dev = (rd[0], rd[0].clone())
        ia = info
    a.close(); d.close()


@pytest.mark.gpu
def test_sharded_handle_is_refused():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import check, GvecError
    eng = g.VecEngine(16, 8, 8, 2, devices=[0, 0], auto_reset=True)
    t = _z(16 * 2 * 9 * 64 * 8, torch.uint8)
    with pytest.raises(GvecError, match="one device"):
        check(eng.L.gvec_gym_observe_players(eng.h, 3, t.data_ptr(), 10, t.data_ptr(), t.data_ptr(), None, None, None))
    with pytest.raises(GvecError, match="one device"):
        check(eng.L.gvec_gym_step_players(eng.h, 3, 1, t.data_ptr(), t.data_ptr(), t.data_ptr(), 10, t.data_ptr(), t.data_ptr(),
                                          *([None] * 9)))
    eng.close()


# ---- CPU: argument checks, no host path ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from generalsreinforcementlearning_amd.csrc import build as Bd
    Bd.build(verbose=False)
    import generalsreinforcementlearning_amd as g
    return g.load()


def _err(L):
    return (L.gvec_last_error() or b"").decode()


def test_selfplay_calls_reject_bad_arguments_without_a_device(lib):
    L = lib
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    obs_args = lambda h, bits, tc, obs, mask: L.gvec_gym_observe_players(h, bits, tc, 10, obs, mask, None, None, None)
    step_args = lambda h, bits, ga, rs, tc, obs, mask: L.gvec_gym_step_players(h, bits, 1, ga, rs, tc, 10, obs, mask, *([None] * 9))
    # learners = 0 and bits at or above GVEC_MAX_PLAYERS are refused before anything else
    for bits in (0, 1 << 8, 1 << 31):
        assert obs_args(p, bits, p, p, p) == -1 and "learners" in _err(L)
        assert step_args(p, bits, p, p, p, p, p) == -1 and "learners" in _err(L)
    # a null handle, null required pointers, max_turns < 1
    assert obs_args(None, 1, p, p, p) == -1 and "null" in _err(L)
    assert step_args(None, 1, p, p, p, p, p) == -1 and "null" in _err(L)
    for k in range(3):
        ptrs = [p, p, p]
        ptrs[k] = None
        assert obs_args(None, 1, *ptrs) == -1 and "null" in _err(L)
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert step_args(None, 1, *ptrs) == -1 and "null" in _err(L)
    assert L.gvec_gym_observe_players(None, 1, p, 0, p, p, None, None, None) == -1 and "max_turns" in _err(L)


def test_selfplay_env_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from generalsreinforcementlearning_amd import GvecError
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    with pytest.raises(GvecError):
        GeneralsSelfPlayVecEnv(4, board_width=8, board_height=8)
