"""rewards_config_kernel and snapshot_rewards_kernel on every compiled <players, slots, parity> variant, on the aged ragged
batches every other board kernel is held to (tests/test_state_forms.py): envs smaller than the handle and with fewer seats,
armies in the int32 escape block, re-deals that change an env's size, and one handle alternating between the full and the
reward-only snapshot.  Everything is compared with tolerance 0, floats as bits, with the numpy restatement of
CalculateRewardWithConfig (tests/_reward_reference.py) on the CPU oracle's states: the build uses -ffp-contract=off and both
sides are the same sequence of IEEE single-precision operations on exact integers.

The first test needs no device: it keeps the oracle runs holding what the device tests then assert they held."""
import ctypes as C

import numpy as np
import pytest

import _harness as H
import _reward_cases as RC
import _reward_reference as R
import _state_forms as F

GUARD = 7


def _gpu():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def _configs():
    from generalsreinforcementlearning_amd import RewardConfig
    return RC.configs(RewardConfig)


# ---- without a device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxp", [2, 4, 8])
def test_variant_runs_hold_every_event_on_the_oracle(maxp):
    """The oracle alone over the twelve runs of one handle limit, the events counted from the restatement's go_default terms:
    every run changes territory, armies, cities and the army advantage and holds armies above 65,535; each of the two small
    runs also loses cities, takes generals, ends games both ways, re-deals envs to another size and has an army difference
    above 2^24.  Every run ends with envs dealt another size after the snapshot whose turn counter still went up: the
    restatement gives them 0 by their dims."""
    cfg = _configs()["go_default"]
    for slots, parity in sorted(H.VARIANT_DIMS):
        ctx = f"<{maxp},{slots},{parity}>"
        _, ora, seed, batch = RC.variant_case(None, maxp, slots, parity)
        tally = RC.play_variant(ora, seed, cfg)
        tally.assert_case_floors(ctx)
        if slots == 1:
            tally.assert_maxp_floors(ctx)
        acts, prev = RC.resize_after_snapshot([ora], ora, batch, seed, lambda: None)
        ora.step(acts)
        cur = ora.read_state(fields=RC.STATE)
        resized = RC.resized_with_turn_up(prev, cur)
        r, t, _ = R.reward_reference(prev, cur, cfg)
        assert resized.sum() >= RC.VARIANT_B // 2 and not r[resized].any() and not t[resized].any(), ctx
        assert t[~resized].any(), f"{ctx}: the envs that kept their size are compared"


# ---- 1. every compiled variant ----------------------------------------------------------------------------------------------
def _raw_call(eng, cfg_c, rewards=None, terms=None, done=None):
    """gvec_experience_rewards_config for all seats into host arrays, any of the three outputs left out (NULL)"""
    from generalsreinforcementlearning_amd._lib import check
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    check(eng.L.gvec_experience_rewards_config(eng.h, C.byref(cfg_c), 0, None, p(rewards), p(terms), p(done), 0), "gvec_experience_rewards_config")


@pytest.mark.gpu
@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_configured_rewards_on_aged_envs(maxp, slots, parity):
    """60 lock-step turns; the snapshot is the full one on odd turns and the reward-only one on even turns of the same handle.
    Every turn: the fixed-weight entry point == the configured one with go_default == the restatement; the "awkward" and
    the "clip" config (with refused actions) == the restatement, rewards, terms and done.  Every fifth turn: seat subsets ==
    the matching columns of the all-seats call, a seat the env does not have reads 0, and each output alone == the full call.
    Last, envs dealt another size between the snapshot and the step, with a turn counter that still went up."""
    g = _gpu()
    eng, ora, seed, batch = RC.variant_case(g, maxp, slots, parity)
    cfgs = _configs()
    B, ctx = eng.B, f"<{maxp},{slots},{parity}>"
    rng = np.random.default_rng(seed)

    def before_step(k):
        eng.experience_begin(rewards_only=(k % 2 == 0))

    def after_step(k, acts, err, prev, cur, want):
        assert np.array_equal(eng.step(acts), err), f"{ctx} turn {k}: error codes differ"
        r_old, d_old = eng.experience_rewards()
        got = eng.experience_rewards(config=cfgs["go_default"], terms=True)
        assert r_old.tobytes() == got[0].tobytes() and np.array_equal(d_old, got[1]), f"{ctx} turn {k}: the two entry points differ"
        RC.assert_equals_restatement(got, prev, cur, cfgs["go_default"], None, f"{ctx} turn {k} go_default", want)
        for cname in ("awkward", "clip"):
            inv = (rng.random((B, maxp)) < 0.1) if cname == "clip" else None
            got = eng.experience_rewards(config=cfgs[cname], invalid=inv, terms=True)
            RC.assert_equals_restatement(got, prev, cur, cfgs[cname], inv, f"{ctx} turn {k} {cname}")
        if k % 5:
            return
        ra, da, ta = eng.experience_rewards(config=cfgs["awkward"], terms=True)
        absent = np.arange(maxp)[None] >= cur["players"][:, None]
        assert not RC.bits(ra)[absent].any() and not ta[absent].any(), f"{ctx} turn {k}: a seat the env does not have"
        for subset in RC.SUBSETS[maxp]:
            ids = RC.seat_ids(subset, maxp)
            rs, ds, ts = eng.experience_rewards(config=cfgs["awkward"], players=subset, terms=True)
            assert rs.shape == (B, len(ids)) and ts.shape == (B, len(ids), 8)
            assert rs.tobytes() == np.ascontiguousarray(ra[:, ids]).tobytes(), f"{ctx} turn {k}: rewards of seats {subset}"
            assert ts.tobytes() == np.ascontiguousarray(ta[:, ids]).tobytes(), f"{ctx} turn {k}: terms of seats {subset}"
            assert np.array_equal(ds, da)
        cfg_c = cfgs["awkward"].to_c()
        r1, t1, d1 = np.full((B, maxp), GUARD, np.float32), np.full((B, maxp, 8), GUARD, np.int32), np.full(B, GUARD, np.uint8)
        _raw_call(eng, cfg_c, terms=t1)
        _raw_call(eng, cfg_c, done=d1)
        _raw_call(eng, cfg_c, rewards=r1)
        assert r1.tobytes() == ra.tobytes() and t1.tobytes() == ta.tobytes() and np.array_equal(d1, da), f"{ctx} turn {k}: one output alone"

    tally = RC.play_variant(ora, seed, cfgs["go_default"], before_step, after_step)
    st = eng.game_state()
    H.assert_states_equal(st, ora.read_state(), f"{ctx} at the end")        # the reward launches changed no board
    F.check_flag_invariants(eng, st, f"{ctx} at the end")
    tally.assert_case_floors(ctx)
    if slots == 1:
        tally.assert_maxp_floors(ctx)
    # envs dealt another size after the snapshot, their turn counter above the snapshot's: the snapshot's dims say "no predecessor"
    for lean in (False, True):
        acts, prev = RC.resize_after_snapshot([eng, ora], ora, batch, seed + int(lean), lambda: eng.experience_begin(rewards_only=lean))
        assert np.array_equal(eng.step(acts), ora.step(acts))
        cur = ora.read_state(fields=RC.STATE)
        assert RC.resized_with_turn_up(prev, cur).sum() >= B // 2
        for cname in ("go_default", "awkward"):
            RC.assert_equals_restatement(eng.experience_rewards(config=cfgs[cname], terms=True), prev, cur, cfgs[cname], None,
                                         f"{ctx} resized after the {'reward-only' if lean else 'full'} snapshot, {cname}")
        r_old, _ = eng.experience_rewards()
        assert r_old.tobytes() == eng.experience_rewards(config=cfgs["go_default"])[0].tobytes()
    st = eng.game_state()
    H.assert_states_equal(st, ora.read_state(), f"{ctx} after the resets")
    F.check_flag_invariants(eng, st, f"{ctx} after the resets")
    eng.close()


# ---- 2. the device-memory path, guarded -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,P,B,masks", [(16, 16, 8, 70, (0b10000000, 0b10010010, 0)), (5, 5, 2, 1, (0b10, 0))], ids=["16x16_p8", "5x5_p2"])
def test_device_memory_outputs_stay_inside_their_rows(w, h, P, B, masks):
    """experience_rewards_device into torch buffers with three guard elements before and after each output, so that no output
    starts at more than its element's alignment, and an `invalid` array one byte into its allocation: the payload is the
    host-memory call's, every guard survives.  B = 70 leaves the last workgroup partly filled."""
    import torch
    g = _gpu()
    eng = g.VecEngine(B, w, h, P, auto_reset=True, stream=torch.cuda.current_stream().cuda_stream)
    eng.reset_generated(9)
    eng.build_board_pool(8, 3)
    eng.rollout(30, 5, 20, fused=True, want_stats=False)
    cfg = _configs()["clip"]
    rng = np.random.default_rng(B)
    nonzero = 0
    for k, mask in enumerate(masks * 2):
        K = bin(mask).count("1") if mask else P
        eng.experience_begin(rewards_only=bool(k % 2))
        eng.step(eng.agent_actions(11 + k, 6))
        inv = (rng.random((B, K)) < 0.3).astype(np.uint8)
        want_r, want_d, want_t = eng.experience_rewards(config=cfg, players=mask, invalid=inv, terms=True)
        d_inv = torch.full((B * K + 2,), GUARD, dtype=torch.uint8, device="cuda")
        d_inv[1:1 + B * K] = torch.from_numpy(inv.reshape(-1)).cuda()
        r = torch.full((B * K + 6,), float(GUARD), dtype=torch.float32, device="cuda")
        t = torch.full((B * K * 8 + 6,), GUARD, dtype=torch.int32, device="cuda")
        d = torch.full((B + 6,), GUARD, dtype=torch.uint8, device="cuda")
        eng.experience_rewards_device(cfg.to_c(), mask, d_inv[1:].data_ptr(), r[3:].data_ptr(), t[3:].data_ptr(), d[3:].data_ptr())
        eng.synchronize()
        torch.cuda.synchronize()
        for name, flat, size, want in (("rewards", r, B * K, want_r), ("terms", t, B * K * 8, want_t), ("done", d, B, want_d.astype(np.uint8))):
            got = flat.cpu().numpy()
            assert (got[:3] == GUARD).all() and (got[3 + size:] == GUARD).all(), f"mask {mask:#x}: a store outside {name}"
            assert got[3:3 + size].tobytes() == np.ascontiguousarray(want).tobytes(), f"mask {mask:#x}: {name}"
        assert (d_inv.cpu().numpy()[[0, -1]] == GUARD).all()
        nonzero += int(np.count_nonzero(want_t))
    assert nonzero > 0
    eng.close()
