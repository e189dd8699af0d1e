"""tests/_memory_reference.py, the numpy restatement of the fog-of-war memory planes, against planes written out by hand: a
2x2 board over five updates (visible, hidden, hidden, a reset, visible again) and the saturation of age at cap = 2."""
import numpy as np

import _memory_reference as R

F = np.float32


def _obs(vis, owner, army):
    """one row's observation of a 2x2 board from three 4-tile lists; planes 3-8, which the update must not read, hold NaN"""
    o = np.full((1, 9, 2, 2), np.nan, F)
    for p, v in enumerate((vis, owner, army)):
        o[0, p] = np.array(v, F).reshape(2, 2)
    return o


def _planes(seen, owner, army, age):
    return np.array([seen, owner, army, age], F).reshape(1, 4, 2, 2)


def test_blank_row():
    assert np.array_equal(R.blank(1, 2, 2), _planes([0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]))


def test_five_updates_by_hand():
    cap = 4
    a, b, c, d, e = F(0.3), F(0.2), F(0.1), F(0.25), F(0.35)
    steps = [
        # tiles 0, 1 and 3 are seen; tile 2 never is
        (_obs([1, 1, 0, 1], [1.0, 0.5, 0, 0], [a, b, 0, c]), None,
         _planes([1, 1, 0, 1], [1.0, 0.5, 0, 0], [a, b, 0, c], [0, 0, 1, 0])),
        # hidden: tiles 0 and 3 keep what they showed and age; tile 1 stays in sight with another army
        (_obs([0, 1, 0, 0], [0, 0.5, 0, 0], [0, d, 0, 0]), [0],
         _planes([1, 1, 0, 1], [1.0, 0.5, 0, 0], [a, d, 0, c], [0.25, 0, 1, 0.25])),
        # hidden again
        (_obs([0, 1, 0, 0], [0, 0.5, 0, 0], [0, d, 0, 0]), [0],
         _planes([1, 1, 0, 1], [1.0, 0.5, 0, 0], [a, d, 0, c], [0.5, 0, 1, 0.5])),
        # the env was re-dealt: everything remembered goes, then the observation applies
        (_obs([0, 1, 0, 0], [0, 0.5, 0, 0], [0, d, 0, 0]), [1],
         _planes([0, 1, 0, 0], [0, 0.5, 0, 0], [0, d, 0, 0], [1, 0, 1, 1])),
        # visible again: tile 0 comes back with what it shows now; tile 1 is hidden for the first time
        (_obs([1, 0, 0, 0], [1.0, 0, 0, 0], [e, 0, 0, 0]), [0],
         _planes([1, 1, 0, 0], [1.0, 0.5, 0, 0], [e, d, 0, 0], [0, 0.25, 1, 1])),
    ]
    state = None
    for i, (obs, reset, want) in enumerate(steps):
        before = None if state is None else state.copy()
        got = R.update(state, obs, reset, cap)
        assert got.dtype == np.float32 and np.array_equal(got, want), (i, got)
        if before is not None:
            assert np.array_equal(state, before)                         # the arguments are left unchanged
        state = got
    seq = R.run(np.stack([s[0] for s in steps]), [s[1] for s in steps], cap)
    assert np.array_equal(seq, np.stack([s[2] for s in steps]))


def test_age_saturates_at_cap_2():
    seen_once = _obs([1, 0, 0, 0], [1.0, 0, 0, 0], [F(0.5), 0, 0, 0])
    hidden = _obs([0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0])
    seq = R.run(np.stack([seen_once, hidden, hidden, hidden, hidden]), cap=2)
    assert [float(v) for v in seq[:, 0, R.AGE, 0, 0]] == [0.0, 0.5, 1.0, 1.0, 1.0]
    assert (seq[:, 0, R.SEEN, 0, 0] == 1.0).all() and (seq[:, 0, R.LAST_OWNER, 0, 0] == 1.0).all()   # age 1.0 with seen 1
    assert (seq[:, 0, R.LAST_ARMY, 0, 0] == F(0.5)).all()
    assert (seq[:, 0, R.AGE, 0, 1] == 1.0).all() and (seq[:, 0, R.SEEN, 0, 1] == 0.0).all()


def test_rows_per_flag_and_bit_copies():
    rng = np.random.default_rng(0)
    obs, _ = R.random_sequence(rng, 2, 4, 3, 3, rows_per_flag=2)
    first = R.update(None, obs[0])
    second = R.update(first, obs[1], np.array([1, 0], np.uint8), rows_per_flag=2)
    assert np.array_equal(second[:2], R.update(None, obs[1][:2]))        # rows 0 and 1 share flag 0
    assert np.array_equal(second[2:], R.update(first[2:], obs[1][2:]))
    odd = obs[0].copy()
    odd[:, 1].view(np.uint32)[...] = 0x7FC12345                          # a NaN with a payload: copied, not computed with
    odd[:, 0] = 1.0
    got = R.update(None, odd)
    assert (got[:, R.LAST_OWNER].view(np.uint32) == 0x7FC12345).all()
