"""The turn's fixed-pattern cross-lane moves (GVEC_XLANE, gvec_device.hpp): shared planes to every row, row 0 to every
row, the OR / sum over rows, a row's last lane, a plane's dwords as a lane mask.  Each has an LDS spelling (ds_bpermute /
ds_swizzle) and a vector-ALU one (v_permlane16/32_swap, DPP row_newbcast, v_readlane); the device self-test holds one to
the other, the tests below hold whichever the library was built with to the oracle on every compiled layout, turn by turn,
and the two kernels that share the code to each other."""
import numpy as np
import pytest

import _harness as H
import _oracle as O
import _state_forms as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import generalsreinforcementlearning_amd as g
    g.load()
    return g


def test_selftest_holds_both_spellings(g):
    assert g.lib().gvec_selftest(0) == 0, g.lib().gvec_last_error()


@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_lockstep_from_turn_zero_on_every_variant(g, maxp, slots, parity):
    """60 turns from turn 0 - both growth turns (25, 50), the full fog pass of turn 0 and the incremental ones after it - with
    fog, masks and a share of unchecked moves (aborted turns, list planes), on the smallest boards that select the variant:
    error codes, masks and the full state every turn."""
    B = 8
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    army, owner, typ, w, h, p = H.gen_boards(300 + slots, sizes, mw, mh)
    eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True)
    ora = O.OracleBatch(B, mw, mh, maxp, fog=True)
    eng.reset(army, owner, typ, w, h, p)
    ora.reset(army, owner, typ, w, h, p)
    assert (ora.read_state(fields=("turn",))["turn"] == 0).all()
    H.run_lockstep(eng, ora, 60, seed=5, invalid_permille=20, check_every=1, want_mask=True, ctx=f"<{maxp},{slots},{parity}>")


@pytest.mark.parametrize("maxp,slots,parity", [(4, 7, "odd"), (8, 16, "even")], ids=["4x7", "8x16"])
def test_lockstep_on_wide_armies_and_desynced_lists(g, maxp, slots, parity):
    """The general stats pass (the list sums over int32 armies) and the list planes: envs with planted wide armies and with
    OwnedTiles that differ from ownership (tests/_state_forms.py), 30 turns, everything compared every turn."""
    B, seed = 12, 50 + slots
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = F.aged_pair(g, mw, mh, maxp, sizes, seed)
    st = eng.game_state()
    assert F.wide_envs(st).any() and F.desynced_envs(st).any(), "the aged batch holds neither form"
    H.run_lockstep(eng, ora, 30, seed, invalid_permille=20, check_every=1, want_mask=True, ctx=f"aged <{maxp},{slots},{parity}>")
    F.check_flag_invariants(eng, eng.game_state(), f"aged <{maxp},{slots},{parity}>")


@pytest.mark.parametrize("slots,parity", [(7, "odd"), (10, "even")], ids=["4x7", "4x10"])
def test_per_turn_and_fused_rollouts_agree(g, slots, parity):
    """step_kernel (one turn a launch) and rollout_kernel (40 turns in registers) share every idiom: from the same boards
    they must leave the same state and the same masks."""
    B, maxp = 64, 4
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    army, owner, typ, w, h, p = H.gen_boards(700 + slots, sizes, mw, mh)
    out = []
    for fused in (False, True):
        eng = g.VecEngine(B, mw, mh, maxp, fog_of_war=True, auto_reset=True)
        eng.reset(army, owner, typ, w, h, p)
        eng.build_board_pool(8, 13, w[:8], h[:8], p[:8])
        eng.rollout(40, 9, 20, fused=fused, want_stats=False)
        out.append((eng.game_state(), eng.legal_action_mask_bits()))
    (s0, m0), (s1, m1) = out
    assert sorted(s0) == sorted(s1)
    for f in s0:
        assert np.array_equal(s0[f], s1[f]), f"<4,{slots}>: field '{f}' differs between the per-turn and the fused rollout"
    assert np.array_equal(m0, m1), f"<4,{slots}>: masks differ between the per-turn and the fused rollout"
