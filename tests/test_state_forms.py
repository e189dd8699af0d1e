"""Every board kernel on aged batches: envs whose armies live in the int32 escape block (HF_WIDE), envs whose OwnedTiles
lists differ from ownership (HF_LDIFF), envs at the largest narrow sums, and envs crossing between the forms in both
directions (tests/_state_forms.py plants them).  Each kernel family is held to the reference it already has, value for
value (float outputs as bits), and after every launch that writes boards the header flags must still say what the boards
are (check_flag_invariants).  The first test needs no device: it keeps the planted values producing every form."""
import numpy as np
import pytest

import _gym_reference as G
import _harness as H
import _oracle as O
import _state_forms as F

TURNS = 500  # the parity protocol's length (tests/test_hip_protocol.py)


# ---- without a device -------------------------------------------------------------------------------------------------
def test_aged_batch_reaches_every_form_on_the_oracle():
    """The oracle alone plays an aged batch for the protocol's turn count: envs must go narrow -> wide, wide -> narrow,
    and hold lists that differ from ownership.  Guards the planted values against drift."""
    B = 60
    sizes = [[(10, 10, 2), (15, 15, 2), (20, 20, 4), (25, 25, 8)][i % 4] for i in range(B)]
    army, owner, typ, ws, hs, ps = H.gen_boards(31, sizes, 25, 25)
    ora = O.OracleBatch(B, 25, 25, 8)
    ora.reset(army, owner, typ, ws, hs, ps)
    for _ in range(8):
        ora.step(ora.agent_actions(3, 60))
    F.age_batch(ora, 31)
    st = ora.read_state()
    assert F.wide_envs(st)[F.ESCAPE::6].all() and F.wide_envs(st)[F.HUGE::6].all() and not F.wide_envs(st)[F.SATURATED::6].any()
    assert (st["army"][F.SATURATED::6][st["owner"][F.SATURATED::6] >= 0] == F.NARROW_MAX).all()
    tally = F.FormsTally()
    tally.add(st)
    for k in range(TURNS):
        ora.step(ora.agent_actions(3, 60 if k < 40 else 8))
        tally.add(ora.read_state(fields=("army", "owner", "listed")))
    c = tally.counts()
    assert c["to_wide"] >= 10 and c["to_narrow"] >= 5 and c["ldiff"] >= 20, c
    assert (ora.read_state(fields=("army_count",))["army_count"].astype(np.int64) < 2 ** 31 - 1).all()


def _gpu():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


# ---- 1. the per-turn agent step (the benchmarked path) over every compiled layout --------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_per_turn_agent_step_on_aged_envs(maxp, slots, parity):
    """gvec_rollout(1, fused=0) (step_kernel<AGENT=true>) against the oracle agent and turn: error codes, moves, full state
    and legal masks every turn, flags every turn; then the fused rollout over the same turns == the per-turn one."""
    g = _gpu()
    B, turns, seed = 54, 90, 40 + slots
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = F.aged_pair(g, mw, mh, maxp, sizes, seed)
    ctx = f"<{maxp},{slots},{parity}>"
    tally = F.FormsTally()
    tally.add(eng.game_state())
    eng.record_agent_actions(True)
    for k in range(turns):
        permille = 60 if k < 30 else 8
        eng.rollout(1, seed, permille, fused=False, want_stats=False)
        acts = ora.agent_actions(seed, permille)
        err = ora.step(acts)
        assert np.array_equal(eng.last_errors(), err), f"{ctx} turn {k}: error codes differ in envs {np.flatnonzero(eng.last_errors() != err)[:8]}"
        assert np.array_equal(eng.recorded_actions(), acts), f"{ctx} turn {k}: agent moves differ"
        st = eng.game_state()
        H.assert_states_equal(st, ora.read_state(), f"{ctx} after turn {k + 1}")
        assert np.array_equal(eng.legal_action_mask_bits(), ora.legal_mask()), f"{ctx} masks after turn {k + 1}"
        F.check_flag_invariants(eng, st, f"{ctx} step_kernel turn {k + 1}")
        tally.add(st)
    eng.record_agent_actions(False)
    tally.assert_all_seen(ctx)
    # the fused kernel over the same 8 + 30 + 60 turns from the same boards
    army, owner, typ, ws, hs, ps = H.gen_boards(seed, sizes, mw, mh)
    fus = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True)
    fus.reset(army, owner, typ, ws, hs, ps)
    pool = min(16, B)
    fus.build_board_pool(pool, 70 + seed, ws[:pool], hs[:pool], ps[:pool])
    fus.rollout(8, seed, 80, fused=False, want_stats=False)
    F.age_batch(fus, seed)
    fus.rollout(30, seed, 60, fused=True, want_stats=False)
    F.check_flag_invariants(fus, fus.game_state(), f"{ctx} rollout_kernel")
    fus.rollout(turns - 30, seed, 8, fused=True, want_stats=False)
    sf = fus.game_state()
    H.assert_states_equal(sf, st, f"{ctx} fused vs per-turn")
    F.check_flag_invariants(fus, sf, f"{ctx} rollout_kernel")


# ---- 2. gym, one learner: gvec_gym_step == the four-call composition --------------------------------------------------
class _GymSide:
    def __init__(self, g, w, h, P, fog, B, max_turns, seed, production=(1, 1, 1), normal_growth_interval=25):
        import torch
        from generalsreinforcementlearning_amd._lib import check
        dev = torch.device("cuda")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.check, self.B, self.max_turns, n = check, B, max_turns, w * h
        self.e = g.VecEngine(B, w, h, P, fog_of_war=fog, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream,
                             production=production, normal_growth_interval=normal_growth_interval)
        self.e.reset_generated(77 + seed)
        self.e.build_board_pool(16, 5)
        self.e.rollout(8, seed, 80, fused=False, want_stats=False)      # lists that differ from ownership
        F.age_batch(self.e, seed)
        self.turn, self.obs, self.mask = z(B, torch.int64), z((B, 9, n), torch.float32), z((B, n * 5), torch.uint8)
        self.out = {k: z(B, dt) for k, dt in (("reward", torch.float64), ("terminated", torch.uint8), ("truncated", torch.uint8),
                                              ("winner", torch.int8), ("needs_reset", torch.uint8), ("turn_out", torch.int64),
                                              ("played", torch.uint8), ("invalid", torch.uint8), ("error", torch.uint8))}
        self.resetting = z(B, torch.uint8)
        self.acts = z((B, P, 8), torch.uint8)
        e = self.e
        check(e.L.gvec_gym_observe(e.h, 0, self.turn.data_ptr(), max_turns, self.obs.data_ptr(), self.mask.data_ptr(), None, None, None))

    def outputs(self):
        import torch
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy().copy() for k, v in self.out.items()}
        d["obs"], d["mask"], d["turn"] = self.obs.cpu().numpy().view(np.uint32).copy(), self.mask.cpu().numpy().copy(), self.turn.cpu().numpy().copy()
        return d


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog", [(9, 8, 2, True), (20, 20, 4, True), (12, 13, 3, False), (32, 32, 8, True), (25, 24, 8, True)],
                         ids=["9x8_p2", "20x20_p4", "12x13_p3_nofog", "32x32_p8", "25x24_p8"])
def test_gym_step_equals_the_four_call_composition_on_aged_envs(w, h, P, fog):
    """gvec_gym_step (gym_step_kernel) against gvec_agent_actions -> gvec_gym_actions -> gvec_step -> gvec_gym_finish_step
    on a twin aged identically: every output bit for bit every step, flags after every launch, the states at the end."""
    tally, seen = gym_composition_run(w, h, P, fog)
    tally.assert_all_seen(f"gym {w}x{h}")
    assert seen["trunc"] > 0 and seen["reset"] > 0, seen


def gym_composition_run(w, h, P, fog, steps=100, production=(1, 1, 1), normal_growth_interval=25):
    """the comparison itself, under a production config -> (the forms met, the truncations and re-deals met)"""
    import torch
    g = _gpu()
    from generalsreinforcementlearning_amd._lib import check
    B, max_turns, n = 64, 40, w * h
    cfg = dict(production=production, normal_growth_interval=normal_growth_interval)
    one, four = _GymSide(g, w, h, P, fog, B, max_turns, 3, **cfg), _GymSide(g, w, h, P, fog, B, max_turns, 3, **cfg)
    H.assert_states_equal(one.e.game_state(), four.e.game_state(), "twins")
    rng = np.random.default_rng(8)
    tally = F.FormsTally()
    seen = {"trunc": 0, "reset": 0, "reset_wide": 0}
    for k in range(steps):
        mask = one.mask.cpu().numpy().astype(bool)
        acts = np.array([rng.choice(np.flatnonzero(m)) if m.any() else 0 for m in mask], np.int64)
        if k % 3 == 0:
            for e_ in range(8, 40):
                hm = np.flatnonzero(mask[e_][4::5])
                if len(hm):
                    acts[e_] = int(hm[rng.integers(0, len(hm))]) * 5 + 4
        if k % 4 == 1:
            acts[:3] = [int(np.flatnonzero(~m)[rng.integers(0, 10)]) for m in mask[:3]]
        ta = torch.from_numpy(acts).cuda()
        seed = 1000 * k + 3
        wide_before = F.wide_envs(one.e.game_state(fields=("army",)))
        rs = one.resetting.cpu().numpy().astype(bool)
        o, e = one.out, one.e
        prev_mask_four = four.mask.clone()
        check(e.L.gvec_gym_step(e.h, 0, seed, ta.data_ptr(), one.resetting.data_ptr(), one.turn.data_ptr(), max_turns, one.obs.data_ptr(),
                                one.mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(), o["truncated"].data_ptr(),
                                o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr(), o["played"].data_ptr(),
                                o["invalid"].data_ptr(), o["error"].data_ptr()), "gvec_gym_step")
        o, e = four.out, four.e
        check(e.L.gvec_agent_actions(e.h, seed, 0, four.acts.data_ptr(), 1))
        check(e.L.gvec_gym_actions(e.h, 0, ta.data_ptr(), prev_mask_four.data_ptr(), four.resetting.data_ptr(), four.acts.data_ptr(),
                                   o["played"].data_ptr(), o["invalid"].data_ptr(), o["error"].data_ptr()))
        e.step_device(four.acts.data_ptr())
        check(e.L.gvec_gym_finish_step(e.h, 0, four.turn.data_ptr(), max_turns, four.resetting.data_ptr(), o["played"].data_ptr(),
                                       four.obs.data_ptr(), four.mask.data_ptr(), o["reward"].data_ptr(), o["terminated"].data_ptr(),
                                       o["truncated"].data_ptr(), o["winner"].data_ptr(), o["needs_reset"].data_ptr(), o["turn_out"].data_ptr()))
        a, b = one.outputs(), four.outputs()
        for f in a:
            x, y = a[f], b[f]
            if f == "reward":
                x, y = x.view(np.uint64), y.view(np.uint64)
            assert np.array_equal(x, y), (k, f, np.flatnonzero((x != y).reshape(B, -1).any(1))[:8])
        s1, s4 = one.e.game_state(), four.e.game_state()
        H.assert_states_equal(s1, s4, f"gym_step vs composition step {k}")
        F.check_flag_invariants(one.e, s1, f"gym_step_kernel step {k}")
        F.check_flag_invariants(four.e, s4, f"step_kernel step {k}")
        tally.add(s1)
        seen["trunc"] += int(a["truncated"].sum()); seen["reset"] += int(rs.sum()); seen["reset_wide"] += int((rs & wide_before).sum())
        one.resetting.copy_(one.out["needs_reset"])
        four.resetting.copy_(four.out["needs_reset"])
    return tally, seen


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog", [(10, 10, 2, True), (20, 20, 4, True), (16, 16, 3, False)], ids=["10x10_p2", "20x20_p4", "16x16_p3_nofog"])
def test_vec_env_equals_numpy_restatement_on_aged_twins(w, h, P, fog):
    """GeneralsVecEnv(device_outputs=True) against the numpy restatement of the gym env (tests/_gym_reference.py) on a twin
    engine aged the same way: observations, masks, rewards, flags and states, through truncations and re-deals of wide envs."""
    import torch
    g = _gpu()
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    B = 40
    kw = dict(board_width=w, board_height=h, max_players=P, fog_of_war=fog, max_turns=30, seed=5, board_pool=16)
    host = G.NumpyReferenceVecEnv(g.VecEngine(B, w, h, P, fog_of_war=fog, auto_reset=True), B, w, h, max_players=P, fog_of_war=fog,
                                  max_turns=30, seed=5, board_pool=16)
    dev = GeneralsVecEnv(B, device_outputs=True, **kw)
    host.reset()
    dev.reset()
    for env in (host, dev):
        env.engine.rollout(8, 6, 80, fused=False, want_stats=False)
        F.age_batch(env.engine, 6)
    view, host._stats = host._read()
    ho = host._observe(view)
    hi = {"valid_actions_mask": host.valid_actions_mask}
    do, di = dev._reset_device()
    assert np.array_equal(do.cpu().numpy().view(np.uint32), ho.view(np.uint32))
    rng = np.random.default_rng(2)
    tally = F.FormsTally()
    seen = {"trunc": 0, "reset_wide": 0}
    for k in range(100):
        mask = hi["valid_actions_mask"]
        acts = np.array([rng.choice(np.flatnonzero(m)) if m.any() else 0 for m in mask])
        if k % 5 == 2:
            acts[:4] = [int(np.flatnonzero(~m)[rng.integers(0, 20)]) for m in mask[:4]]
        if k % 3 == 0:
            for e in range(8, 24):
                hm = np.flatnonzero(mask[e][4::5])
                if len(hm):
                    acts[e] = int(hm[rng.integers(0, len(hm))]) * 5 + 4
        wide_before = F.wide_envs(dev.engine.game_state(fields=("army",)))
        ho, hr, hterm, htrunc, hi = host.step(acts)
        do, dr, dterm, dtrunc, di = dev.step(torch.from_numpy(acts).cuda())
        assert np.array_equal(do.cpu().numpy().view(np.uint32), ho.view(np.uint32)), k
        assert np.array_equal(di["valid_actions_mask"].cpu().numpy(), hi["valid_actions_mask"]), k
        assert np.array_equal(dr.cpu().numpy().view(np.uint64), np.asarray(hr, np.float64).view(np.uint64)), (k, np.flatnonzero(dr.cpu().numpy() != hr)[:8])
        assert np.array_equal(dterm.cpu().numpy(), hterm) and np.array_equal(dtrunc.cpu().numpy(), htrunc), k
        for f in ("turn", "invalid_action", "error", "winner", "reset"):
            assert np.array_equal(di[f].cpu().numpy(), np.asarray(hi[f])), (k, f)
        st = dev.engine.game_state()
        H.assert_states_equal(st, host.engine.game_state(), f"vec env vs restatement step {k}")
        F.check_flag_invariants(dev.engine, st, f"gym_step_kernel (vec env) step {k}")
        tally.add(st)
        seen["trunc"] += int(htrunc.sum())
        seen["reset_wide"] += int((np.asarray(hi["reset"]).astype(bool) & wide_before).sum())
    assert seen["trunc"] > 0 and seen["reset_wide"] > 0, seen
    tally.assert_all_seen(f"vec env {w}x{h}")
    host.close(); dev.close()


# ---- 3. gym, self-play: every player a learner ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog", [(15, 15, 2, True), (20, 20, 4, True), (32, 32, 8, True), (12, 12, 3, False)],
                         ids=["15x15_p2", "20x20_p4", "32x32_p8", "12x12_p3_nofog"])
def test_self_play_every_learner_on_aged_envs(w, h, P, fog):
    """gvec_gym_step_players / gvec_gym_observe_players with every player a learner against the numpy restatement per
    learner and the oracle turn (tests/test_selfplay_env.py's protocol), on envs aged after a warm-up with invalid moves."""
    self_play_run(w, h, P, fog).assert_all_seen(f"self-play {w}x{h}")


def self_play_run(w, h, P, fog, steps=70, production=(1, 1, 1), normal_growth_interval=25):
    """the comparison itself, under a production config -> the forms met"""
    import test_selfplay_env as SP
    from generalsreinforcementlearning_amd.vec_engine import ACTION_DTYPE
    _gpu()
    B, max_turns, n = SP.B, 30, w * h
    sp = SP.Players(w, h, P, fog, (1 << P) - 1, max_turns, production=production, normal_growth_interval=normal_growth_interval)
    ids, L, eng = sp.ids, len(sp.ids), sp.e
    eng.rollout(8, 12, 80, fused=False, want_stats=False)
    F.age_batch(eng, 12)
    sp.check(eng.L.gvec_gym_observe_players(eng.h, sp.bits, sp.turn.data_ptr(), max_turns, sp.obs.data_ptr(), sp.mask.data_ptr(),
                                            sp.out["reward"].data_ptr(), sp.done0.data_ptr(), sp.out["winner"].data_ptr()))
    ora = O.OracleBatch(B, w, h, P, fog=fog, prod=production, interval=normal_growth_interval)
    st = eng.game_state()
    ora.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])   # the envs write_state fills
    rng = np.random.default_rng(11)
    prev = SP._stats(eng.game_state())
    turn = np.zeros(B, np.int64)
    tally = F.FormsTally()
    for k in range(steps):
        st0 = eng.game_state()
        rs = sp.resetting.cpu().numpy().astype(bool)
        masks0 = []
        for p in ids:
            vis, fog_ = eng.compute_player_visibility(p)
            masks0.append(G.valid_actions_mask(G.proto_view(st0["owner"], st0["army"], st0["type"], vis, fog_), p, w, h))
        acts = SP._learner_actions(rng, masks0, k, n, L, w, h)
        dec = SP._expected_decode(acts, masks0, ids, w, h, st0, rs)
        out = sp.step(acts, 500 + k)
        turn = np.where(rs, 0, turn + 1)
        st1, cur = SP._check_learners(out, eng, ids, dec, prev, rs, turn, w, h, max_turns, f"{w}x{h} step {k}")
        F.check_flag_invariants(eng, st1, f"gym_step_players_kernel step {k}")
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
        tally.add(st1)
        prev = cur
        sp.next_step()
    return tally


# ---- 4. the stream's tile updates (army in bits 32-63 of each row) ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fog", [True, False], ids=["fog_on", "fog_off"])
def test_stream_deltas_on_aged_envs(fog):
    """gvec_stream_deltas and gvec_stream_deltas_packed (full_tiles 0 and 1) against wire.stream_update /
    stream_update_from_delta on the oracle's state, over a padded mixed batch of aged envs."""
    from generalsreinforcementlearning_amd import wire
    g = _gpu()
    B = 48
    per = [[(10, 8, 3), (15, 15, 2), (20, 20, 4), (20, 17, 4)][i % 4] for i in range(B)]
    eng, ora = F.aged_pair(g, 20, 20, 4, per, 17, fog=fog)
    tally = F.FormsTally()
    seen = {1: 0, 2: 0, "wide_rows": 0}
    for k in range(50):
        acts = ora.agent_actions(5, 50 if k < 15 else 10)
        assert np.array_equal(eng.step(acts), ora.step(acts)), k
        st = ora.read_state()
        H.assert_states_equal(eng.game_state(), st, f"stream turn {k}")
        tally.add(st)
        for viewer in (0, 1, 3):
            kind, count, upd = eng.stream_deltas(viewer)
            pk, poff, pupd = eng.stream_deltas_packed(viewer)
            assert np.array_equal(pk, kind) and np.array_equal(np.diff(poff), count) and poff[0] == 0
            assert np.array_equal(pupd, np.concatenate([upd[e_, : count[e_]] for e_ in range(B)]))
            fk, foff, fupd = eng.stream_deltas_packed(viewer, full_tiles=True)
            assert np.array_equal(fk, kind)
            vis, fg = eng.compute_player_visibility(viewer)
            for e in range(B):
                w, h, P = per[e]
                if viewer >= P:
                    continue
                want = wire.stream_update(st, vis, fg, np.zeros(w * h * 4, bool), e, viewer)
                got = wire.stream_update_from_delta(st, kind, count, upd, e, viewer)
                seen[int(kind[e])] += 1
                mine = fupd[foff[e]: foff[e + 1]]
                seen["wide_rows"] += int(((mine >> np.uint64(32)).astype(np.uint32).view(np.int32) > F.NARROW_MAX).sum())
                if want.WhichOneof("update") == "full_state":
                    assert kind[e] == 2 and got is None and count[e] == 0, (k, e, viewer)
                    assert len(mine) == w * h
                    assert wire.full_state_from_tiles(st, mine, np.zeros(w * h * 4, bool), e, viewer) == want.full_state, (k, e, viewer)
                else:
                    assert np.array_equal(mine, upd[e, : count[e]])
                    assert kind[e] == 1 and got is not None, (k, e, viewer)
                    want.ClearField("timestamp")
                    got.ClearField("timestamp")
                    assert got == want, (k, e, viewer)
    tally.assert_all_seen("stream")
    assert seen[1] > 100 and seen[2] > 10 and seen["wide_rows"] > 0, seen


# ---- 5. the experience side channel ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,fog", [(15, 15, 2, True), (20, 20, 4, True), (32, 32, 8, True), (16, 16, 3, False)],
                         ids=["15x15_p2", "20x20_p4", "32x32_p8", "16x16_p3_nofog"])
def test_experience_channel_on_aged_envs(w, h, P, fog):
    """gvec_observe, gvec_serializer_mask and gvec_experience_rewards (float32 on per-player army sums) against the oracle
    every turn; gvec_experience_records expanded by gvec_expand_experience_records against the oracle's own tensors,
    masks and rewards for the same transitions, and the records' armies saturated to u16 as documented."""
    import torch
    from generalsreinforcementlearning_amd.experience import expand_records_device, record_offsets
    from generalsreinforcementlearning_amd.vec_engine import unpack_legal_bits
    g = _gpu()
    B = 48
    eng, ora = F.aged_pair(g, w, h, P, [(w, h, P)] * B, 23, fog=fog)
    lay = eng.experience_record_layout()
    off, n = record_offsets(lay), w * h
    slab = torch.zeros(B * lay["record_dw"], dtype=torch.int32, device="cuda")
    tally = F.FormsTally()
    saturated = 0
    for k in range(40):
        acts = ora.agent_actions(41, 50 if k < 10 else 10)
        prev = ora.read_state()
        prev_obs = [ora.observe(p) for p in range(P)]
        prev_mask = ora.serializer_mask()
        eng.experience_begin()
        ora.experience_begin()
        assert np.array_equal(eng.step(acts), ora.step(acts)), k
        cur = ora.read_state()
        H.assert_states_equal(eng.game_state(), cur, f"experience turn {k}")
        F.check_flag_invariants(eng, cur, f"step_kernel turn {k}")
        tally.add(cur)
        hr, hd = eng.experience_rewards()
        orr, od = ora.rewards()
        assert np.array_equal(hr.view(np.uint32), orr.view(np.uint32)), (k, np.argwhere(hr != orr)[:6])
        assert np.array_equal(hd, od.astype(bool)), k
        assert np.array_equal(eng.serializer_mask_bits(), ora.serializer_mask()), k
        cur_obs = [ora.observe(p) for p in range(P)]
        for p in range(P):
            assert np.array_equal(eng.observe(p).view(np.uint32), cur_obs[p].view(np.uint32)), (k, p)
        eng.experience_records(slab.data_ptr(), actions=acts)
        eng.synchronize()
        recs = slab.cpu().numpy().view(np.uint32).reshape(B, lay["record_dw"])
        for name, src in (("army_prev", prev["army"]), ("army_next", cur["army"])):
            a16 = recs[:, off[name]: off[name] + lay["ns"] * 32].view(np.uint16)[:, :n]
            assert np.array_equal(a16, np.clip(src[:, :n], 0, 65535).astype(np.uint16)), (k, name)
            saturated += int((src[:, :n] > 65535).sum())
        ex = expand_records_device(slab, lay)
        envs, pls = ex["env"].cpu().numpy(), ex["player_id"].cpu().numpy()
        comparable = (cur["turn"] > prev["turn"])
        want = [(e, p) for e in range(B) if comparable[e] for p in range(P) if p < cur["players"][e] and acts[e, p]["flags"] & 1]
        assert [(int(e), int(p)) for e, p in zip(envs, pls)] == want, k
        xs, xn, xm = ex["state"].cpu().numpy(), ex["next_state"].cpu().numpy(), ex["action_mask"].cpu().numpy()
        xr, xd = ex["reward"].cpu().numpy(), ex["done"].cpu().numpy()
        for i, (e, p) in enumerate(want):
            assert np.array_equal(xs[i].reshape(-1).view(np.uint32), prev_obs[p][e].view(np.uint32)), (k, e, p, "state")
            assert np.array_equal(xn[i].reshape(-1).view(np.uint32), cur_obs[p][e].view(np.uint32)), (k, e, p, "next_state")
            assert np.array_equal(xm[i].reshape(-1).astype(bool), unpack_legal_bits(prev_mask[e, p], w, h)), (k, e, p, "action_mask")
            assert xr[i].view(np.uint32) == orr[e, p].view(np.uint32) and bool(xd[i]) == bool(od[e]), (k, e, p)
    tally.assert_all_seen(f"experience {w}x{h}")
    assert saturated > 0
