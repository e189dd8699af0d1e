"""Every kernel that plays a turn, under production configs off the defaults (tests/_production_cases.py has the cases and
what each is there to reach; tests/test_production_rules.py holds the oracle to the rule and the batches to their purpose).
Every comparison is equality of integers and bytes: error codes, legal-mask bits, every field of the state, header flags,
search terms.

    step_kernel          lock-step from turn 0 against the oracle, the header flags against the model of the ordinary turn;
                         aged batches with re-deals; planted turns on both sides of t = 65,536
    rollout_kernel       the fused rollout against the oracle's, and the per-turn agent launches against both
    gym kernels          the one-launch step against the four-call composition, the players' step against the oracle turn
    search kernels       the playouts' terms (random and scripted-bot rollouts) against the CPU reference
    the config's travel  export / import of records and VecEnvState save / load / restore, then playing on"""
import numpy as np
import pytest

import _harness as H
import _ordinary_turn as T
import _production_cases as PC
import _search_bot_reference as SBR
import _search_reference as SR
import _state_forms as F
import test_hip_ordinary_turn as OT

pytestmark = pytest.mark.gpu

THREE_RUNS = [(c, v) for c in PC.CASES for v in PC.THREE]
THREE_IDS = [f"{c.id}-p{v[0]}_slots{v[1]}_{v[2]}" for c, v in THREE_RUNS]
CARRIER_RUNS = [(c, v) for c in PC.CARRIERS for v in OT.VARIANTS]
CARRIER_IDS = [f"{c.id}-p{v[0]}_slots{v[1]}_{v[2]}" for c, v in CARRIER_RUNS]
CONFIGS = [PC.BY_ID["3_2_5_i3"], PC.BY_ID["1_1_1_i1"]]
CONFIG_IDS = [c.id for c in CONFIGS]


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


# ---- the per-turn step kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant", THREE_RUNS, ids=THREE_IDS)
def test_step_kernel_under_every_config(g, case, variant):
    """Lock-step from turn 0 (fog, masks, 20 per mille of unchecked moves): error codes, masks and the full state every turn,
    and before every turn the envs the device's header flags send down the ordinary path against the model's."""
    PC.case_run(g, case, variant)


@pytest.mark.parametrize("case,variant", CARRIER_RUNS, ids=CARRIER_IDS)
def test_step_kernel_carrier_configs_on_every_variant(g, case, variant):
    PC.case_run(g, case, variant)


@pytest.mark.parametrize("case", PC.AGED_CASES, ids=[c.id for c in PC.AGED_CASES])
@pytest.mark.parametrize("aged", OT.AGED, ids=["4x7", "8x16"])
def test_step_kernel_on_aged_batches(g, case, aged):
    """Wide armies, lists that differ from ownership, re-deals from the pool and growth turns staggered over the envs."""
    PC.aged_case_run(g, case, aged)


@pytest.mark.parametrize("case", PC.PLANTED, ids=[c.id for c in PC.PLANTED])
def test_step_kernel_across_the_turn_boundaries(g, case):
    """growth_turn's two branches: the same turn planted on both sides, growth turns before and beyond t = 65,536, the last
    interval on the multiply-high path and the first on `%`."""
    PC.case_run(g, case, PC.PLANT_VARIANT)


# ---- the fused rollout and the per-turn agent launches --------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant", THREE_RUNS, ids=THREE_IDS)
def test_rollouts_under_every_config(g, case, variant):
    """rollout_kernel (fused) and step_kernel<AGENT> (one launch a turn, no stats asked) from the same boards against the
    oracle's rollout of the same arguments: state, masks, lifetime counters."""
    out = []
    for fused in (True, False):
        eng, ora = PC.case_pair(g, case, variant)
        stats = eng.rollout(case.turns, PC.SEED, PC.PERMILLE, fused=fused, want_stats=fused)
        st = eng.game_state()
        out.append((eng.counters(), F.header_flags(eng)))
        if fused:
            steps = ora.rollout(case.turns, PC.SEED, PC.PERMILLE)
            want, masks = ora.read_state(), ora.legal_mask()
            assert stats == eng.counters() and stats["env_steps"] == steps, (stats, steps)
            assert stats["games_finished"] == int(want["done"].sum())
        H.assert_states_equal(st, want, f"{case.id} {variant} fused={fused}")
        assert np.array_equal(eng.legal_action_mask_bits(), masks), f"{case.id} {variant} fused={fused}: legal masks differ"
        F.check_flag_invariants(eng, st, f"{case.id} {variant} fused={fused}")
    assert out[0][0] == out[1][0], f"{case.id} {variant}: counters differ between the fused and the per-turn rollout: {out[0][0]} {out[1][0]}"
    assert np.array_equal(out[0][1], out[1][1]), f"{case.id} {variant}: header flags differ between the fused and the per-turn rollout"


# ---- the gym kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("w,h,P", [(9, 8, 2), (20, 20, 4)], ids=["9x8_p2", "20x20_p4"])
def test_gym_step_equals_the_four_call_composition(case, w, h, P):
    """gym_step_kernel against the composition through gvec_step (held to the oracle above), 40 steps."""
    import test_state_forms as SFT
    tally, seen = SFT.gym_composition_run(w, h, P, True, steps=40, production=case.prod, normal_growth_interval=case.interval)
    assert tally.counts()["wide"] > 0 and seen["trunc"] + seen["reset"] > 0, (tally.counts(), seen)


@pytest.mark.parametrize("case", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("w,h,P", [(15, 15, 2), (20, 20, 4)], ids=["15x15_p2", "20x20_p4"])
def test_gym_step_players_equals_the_oracle_turn(case, w, h, P):
    """gym_step_players_kernel with every player a learner against the oracle's turn under the config, 40 steps."""
    import test_state_forms as SFT
    tally = SFT.self_play_run(w, h, P, True, steps=40, production=case.prod, normal_growth_interval=case.interval)
    assert tally.counts()["wide"] > 0, tally.counts()


# ---- the search kernels ---------------------------------------------------------------------------------------------------------
SEARCH_B, SEARCH_R, SEARCH_D, SEARCH_SEED = 6, 2, 6, 11   # depth 6: a growth turn falls inside every playout under intervals 1 and 3


def _search_roots(HS, case):
    mw, mh, sizes = H.variant_batch(*PC.PLANT_VARIANT, SEARCH_B)
    eng, ora = HS._twins(mw, mh, 4, sizes, prod=case.prod, interval=case.interval)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(SEARCH_B) + 1) % st["players"]
    cand = HS._candidates(st, players, mw * mh, True)
    assert (cand[:, 0] >= 0).sum() >= SEARCH_B - 1
    return eng, st, players, cand, mw, mh


@pytest.mark.parametrize("case", PC.CARRIERS, ids=[c.id for c in PC.CARRIERS])
def test_search_playouts_equal_the_reference(case):
    import test_hip_search as HS
    eng, st, players, cand, mw, mh = _search_roots(HS, case)
    want = SR.reference_terms(st, None, players, cand, SEARCH_R, SEARCH_D, SEARCH_SEED, mw, mh, 4, prod=case.prod, interval=case.interval)
    assert (want[:, :4, :, 0] == 1).sum() >= (SEARCH_B - 1) * 4 * SEARCH_R
    HS._assert_terms_equal(HS._terms(eng, None, players, cand, SEARCH_R, SEARCH_D, SEARCH_SEED), want, case.id)
    eng.close()


@pytest.mark.parametrize("case", PC.CARRIERS, ids=[c.id for c in PC.CARRIERS])
def test_search_bot_playouts_equal_the_reference(case):
    import test_hip_search_bot as HSB
    eng, st, players, cand, mw, mh = _search_roots(HSB, case)
    want = SBR.reference_terms_bot(st, None, players, cand, SEARCH_R, SEARCH_D, SEARCH_SEED, mw, mh, 4, 0b1111, prod=case.prod, interval=case.interval)
    assert (want[..., 0] == 1).sum() >= (SEARCH_B - 1) * 3 * SEARCH_R
    HSB._assert_terms_equal(HSB._terms(eng, None, players, cand, SEARCH_R, SEARCH_D, SEARCH_SEED, 0b1111), want, case.id)
    eng.close()


# ---- the config travels with the records ----------------------------------------------------------------------------------------
TRAVEL = PC.BY_ID["3_2_5_i3"]


def _play_on(a, b, turns, ctx, ora=None):
    """both engines a turn at a time with the on-device agent; ora: the oracle plays the same turns with its own agent"""
    for k in range(turns):
        for e in (a, b):
            e.rollout(1, 900 + k, 30, fused=False, want_stats=False)
        assert np.array_equal(a.last_errors(), b.last_errors()), f"{ctx} turn {k}: error codes"
        H.assert_states_equal(a.game_state(), b.game_state(), f"{ctx} turn {k}")
        if ora is not None:
            ora.rollout(1, 900 + k, 30)
            H.assert_states_equal(a.game_state(), ora.read_state(), f"{ctx} turn {k} against the oracle")


def _travel_source(g):
    eng, ora = PC.case_pair(g, TRAVEL, PC.PLANT_VARIANT)
    OT.lockstep(eng, ora, T.FlagModel(ora.read_state()), 10, PC.SEED, PC.PERMILLE, "travel warm-up",
                prod=TRAVEL.prod, interval=TRAVEL.interval)
    return eng, ora


def test_records_exported_and_imported_play_on_under_the_config(g):
    import torch
    src, ora = _travel_source(g)
    slab = torch.empty(src.B * src.state_bytes_per_env(), dtype=torch.uint8, device="cuda")
    src.export_records(slab.data_ptr())
    twin = g.VecEngine(src.B, src.max_w, src.max_h, src.max_p, fog_of_war=True, production=TRAVEL.prod, normal_growth_interval=TRAVEL.interval)
    twin.reset_generated(3)
    twin.import_records(slab.data_ptr())
    H.assert_states_equal(twin.game_state(), ora.read_state(), "imported records")
    _play_on(src, twin, 12, "export / import", ora)    # growth turns 12, 15, 18, 21


def test_env_state_saved_loaded_and_restored_plays_on_under_the_config(g, tmp_path):
    import torch
    from generalsreinforcementlearning_amd import VecEnvState
    src, _ = _travel_source(g)
    B = src.B
    held = g.VecEngine(B, src.max_w, src.max_h, src.max_p, fog_of_war=True, production=TRAVEL.prod, normal_growth_interval=TRAVEL.interval,
                       auto_reset=True)
    held.copy_envs(src=src)
    config = {"board_width": src.max_w, "board_height": src.max_h, "max_players": src.max_p, "fog_of_war": True, "production": list(TRAVEL.prod),
              "normal_growth_interval": TRAVEL.interval, "max_turns": 100, "learners": [0], "num_envs": B}
    z = lambda dt: torch.zeros(B, dtype=dt, device="cuda")
    state = VecEnvState(held, torch.arange(B, device="cuda"), z(torch.int64), z(torch.bool), None, None, config)
    path = tmp_path / "state.npz"
    state.save(str(path))
    loaded = VecEnvState.load(str(path))
    assert loaded.engine.production == TRAVEL.prod and loaded.engine.normal_growth_interval == TRAVEL.interval
    assert loaded.config == config
    restored = g.VecEngine(B, src.max_w, src.max_h, src.max_p, fog_of_war=True, production=TRAVEL.prod, normal_growth_interval=TRAVEL.interval)
    restored.reset_generated(3)
    restored.copy_envs(src=loaded.engine)
    H.assert_states_equal(restored.game_state(), src.game_state(), "restored")
    _play_on(held, loaded.engine, 12, "the loaded engine itself")    # growth turns 12, 15, 18, 21
    _play_on(src, restored, 12, "save / load / restore")
    H.assert_states_equal(restored.game_state(), held.game_state(), "restored against the engine that was saved")
