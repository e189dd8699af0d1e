"""The placements of tests/test_hip_store_paths.py reach every store path of the observation and mask writers.

No device: the paths are computed from the placements, VARIANT_DIMS and the ragged batches of _harness.variant_batch by
the selectors restated in tests/_store_paths.py.  What "every path" means is not a list kept by hand: it is what the
selector yields over ALL addresses the buffer's element alignment allows (_store_paths.reachable), so a placement or a
board shape whose removal makes a path unreachable fails here, before the GPU test could skip the path without a word.

Window offsets: a windowed path must run with sh = 0, 1 and 63 (no shift, the smallest, the largest) wherever the selector
lets that sh reach the windowed path at all - on a board whose planes are a multiple of four floats sh = 0 means an aligned
buffer, which takes the quad or slot path instead - and with a value in between."""
import pytest

import _harness as H
import _store_paths as SP

FULL_SLOT = {(1, "even"): (8, 8), (4, "even"): (16, 16), (16, "even"): (32, 32)}


def test_selectors_on_known_cases():
    """the table against cases worked out by hand from the kernels' code"""
    b = SP.BASE
    assert [SP.nslot_of(w * h) for w, h in (H.VARIANT_DIMS[k] for k in sorted(H.VARIANT_DIMS))] == [k[0] for k in sorted(H.VARIANT_DIMS)]
    # 20x20: aligned -> quads; +12 bytes -> windows, plane p at (3 + 400 p) & 63 = 3 + 16 p (mod 64); 400 + 3 tiles span 7 windows
    assert SP.gym_obs(b, 400, 7) == [("quads", None, None)]
    assert SP.gym_obs(b + 12, 400, 7)[:3] == [("windows", 3, 7), ("windows", 19, 7), ("windows", 35, 7)]
    assert SP.gym_obs(b, 100, 2) == [("slots", None, None)] and SP.gym_obs(b, 225, 4)[1] == ("windows", 225 & 63, 5)
    # 8x8 is one slot: any shift needs the second window, no shift cannot take the windowed path
    assert SP.gym_obs(b + 4, 64, 1) == [("windows", 1, 2)] * 9 and SP.gym_obs(b + 252, 64, 1) == [("windows", 63, 2)] * 9
    assert SP.gym_obs(b + 16, 64, 1) == [("slots", None, None)]
    assert SP.gym_obs(b + 4, 1024, 16)[0] == ("windows", 1, 17)
    # the mask: 5 * 400 = 2000 bytes are whole 16-byte pieces, 5 * 600 = 3000 only whole dwords, 5 * 625 neither
    assert [SP.gym_mask(b + o, 400)[0][0] for o in (0, 16, 4, 2)] == ["16-byte", "16-byte", "4-byte", "byte"]
    assert [SP.gym_mask(b + o, 600)[0][0] for o in (0, 16, 4, 2)] == ["4-byte", "4-byte", "4-byte", "byte"]
    assert [SP.gym_mask(b + o, 625)[0][0] for o in (0, 16, 4, 2)] == ["byte"] * 4
    # observe_kernel: the pitch is the env's own N
    assert SP.observe(b, 256) == [("slots", None, None)] and SP.observe(b + 8, 256) == [("windows", 2, 5)] * 9
    assert SP.observe(b, 400)[:2] == [("windows", 0, 7), ("windows", 16, 7)]
    assert SP.expand_tensor(b, 400) == [("quads", None, None)] and SP.expand_tensor(b + 4, 400)[0] == ("windows", 1, 7)
    assert SP.expand_tensor(b, 225)[2] == ("windows", 450 & 63, 4)
    assert SP.expand_mask(b + 252, 64) == [("windows", 63, 2)] and SP.expand_mask(b, 64) == [("windows", 0, 1)]
    assert SP.store_masks(b)[0][0] == "wide" and SP.store_masks(b + 8)[0][0] == "narrow"


def test_placements_are_the_ones_the_header_allows():
    assert SP.FLOAT_OFFSETS == (0, 4, 8, 12, 16, 252) and SP.BYTE_OFFSETS == (0, 1, 2, 3, 4, 16) and SP.DWORD_OFFSETS == (0, 4, 8, 12)
    assert all(o % 4 == 0 for o in SP.FLOAT_OFFSETS + SP.DWORD_OFFSETS)
    # each output's offsets with the other aligned, one placement with both odd
    assert {p for p in SP.GYM_PLACEMENTS if p[1] == 0} == {(o, 0) for o in SP.FLOAT_OFFSETS}
    assert {p for p in SP.GYM_PLACEMENTS if p[0] == 0} == {(0, o) for o in SP.BYTE_OFFSETS}
    assert [p for p in SP.GYM_PLACEMENTS if p[0] and p[1]] == [(4, 3)] and len(SP.GYM_PLACEMENTS) == 12
    assert len(SP.EXPAND_PLACEMENTS) == 17 and SP.EXPAND_PLACEMENTS[-1] == (4, 4, 4)
    assert all(o % 4 == 0 for p in SP.EXPAND_PLACEMENTS for o in p)


@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_placements_reach_every_path(maxp, slots, parity):
    stride, tiles, players = SP.batch_tiles(maxp, slots, parity)
    ns = SP.nslot_of(stride)
    assert ns == slots and max(tiles) == stride and min(tiles) < stride
    got = SP.promised(maxp, slots, parity, learners=maxp)
    SP.assert_coverage(got, stride, tiles)
    assert ((slots, parity) in FULL_SLOT) == (stride == 64 * ns)
    # the paths the suite ran nowhere, or on one shape only, before these placements
    names = {site: {e[1] for e in got[site]} for site in got}
    assert "windows" in names["gym_emit.obs"] and "windows" in names["observe"] and "windows" in names["expand.tensor"]
    assert "byte" in names["gym_emit.mask"] and (stride % 4 or "4-byte" in names["gym_emit.mask"])
    assert any(n % 64 for n in tiles) or stride % 64 == 0
    if any(n % 64 == 0 for n in tiles):
        assert "slots" in names["observe"]
    if any(n % 4 == 0 for n in tiles):
        assert "quads" in names["expand.tensor"]


@pytest.mark.parametrize("maxp", [2, 4, 8])
def test_the_prepared_state_is_what_the_launches_take_for_granted(maxp):
    """The oracle alone plays and plants the GPU test's batches (the engine must equal it there): no re-deal changes an
    env's size, which the promised paths are computed from, no env sits on a finished game, the seats whose observations
    are compared are alive where the planted armies are, and every 64-tile slot of the largest board holds an army."""
    import _oracle as O
    for slots, parity in sorted(H.VARIANT_DIMS):
        mw, mh = H.VARIANT_DIMS[(slots, parity)]
        ora = O.OracleBatch(SP.B, mw, mh, maxp, fog=True)
        SP.deal(ora, maxp, slots, parity, 900 + slots)
        SP.prepare(ora, 900 + slots)
        st = ora.read_state()
        SP.check_prepared(st, maxp, slots, parity)
        assert (st["type"][SP.WIDE_ENV] == 3).any() and st["turn"].min() >= SP.TURNS


def test_the_three_full_slot_shapes_are_in_the_variant_table():
    full = {k: v for k, v in H.VARIANT_DIMS.items() if v[0] * v[1] == 64 * k[0]}
    assert full == FULL_SLOT


def test_the_wider_mask_paths_meet_the_narrower_on_one_shape():
    """the 4-byte and the byte path of gym_emit's mask run on shapes where the 16-byte path exists too"""
    for (slots, parity), (w, h) in H.VARIANT_DIMS.items():
        got = {e[1] for e in SP.promised(2, slots, parity, learners=2)["gym_emit.mask"]}
        want = {"16-byte", "4-byte", "byte"} if (5 * w * h) % 16 == 0 else {"4-byte", "byte"} if (5 * w * h) % 4 == 0 else {"byte"}
        assert got == want, (w, h, got)
    rows = [5 * w * h for w, h in H.VARIANT_DIMS.values()]
    assert sum(n % 16 == 0 for n in rows) >= 3 and any(n % 16 and n % 4 == 0 for n in rows) and any(n % 4 for n in rows)
