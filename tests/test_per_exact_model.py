"""The exact model of the prioritized-replay tree (_per_exact.py) held to the float64 model (_per_reference.py), and the
coverage of the scripted sequences tests/test_hip_per_exact.py runs on the device.  No GPU."""
import numpy as np
import pytest

import _per_exact as X
import _per_reference as R

SEED = 20


def test_cumsum_is_the_sequential_float32_prefix():
    rng = np.random.default_rng(1)
    c = (10.0 ** rng.uniform(-3, 3, (7, 64))).astype(np.float32)
    c[2, 5:40] = 0
    P = np.cumsum(c, axis=1, dtype=np.float32)
    for row in range(7):
        acc = c[row, 0]
        for j in range(1, 64):
            acc = np.float32(acc + c[row, j])
            assert acc == P[row, j]
        assert X.node_sums(c.reshape(-1))[row] == acc
    # the order matters: this is not the pairwise sum numpy's own `sum` makes
    assert (np.cumsum(c, axis=1, dtype=np.float32)[:, 63] != c.sum(1, dtype=np.float32)).any()


@pytest.mark.parametrize("cap,levels", [(1, 1), (60, 1), (64, 1), (65, 2), (100, 2), (4096, 2), (4097, 3), (5000, 3), (262144, 3), (262145, 4)])
def test_layout(cap, levels):
    L, words, off = X.layout(cap)
    assert L == levels and off[0] == 64
    n, at = cap, 64
    for l in range(L + 1):
        assert off[l] == at
        at += (n + 63) // 64 * 64
        n = (n + 63) // 64
    assert n == 1 and words == at
    t = X.ExactTree(cap)
    assert t.widths[-1] == 64 and sum(t.widths) + 64 == words and t.image().shape == (words,)
    assert t.header() == {0: 0x3F800000, 1: 0, 2: 0, 3: 0, 4: 0x7F800000, 5: 0x7F800000, 6: 0, 7: 0}


def test_u_of_is_53_bits_keyed_by_seed_call_and_draw():
    j = np.arange(4096)
    u = X.u_of(11, 0, j)
    assert u.dtype == np.float64 and (u >= 0).all() and (u <= X.U_TOP).all()
    assert (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()                      # 53-bit fractions
    assert 0.45 < u.mean() < 0.55 and len(np.unique(u)) == 4096
    assert not np.array_equal(u, X.u_of(11, 1, j)) and not np.array_equal(u, X.u_of(12, 0, j))
    assert not np.array_equal(u, X.u_of(11 + (1 << 32), 0, j))                   # the seed's high word counts
    assert X.u_of(11, 0, 5) == u[5] and X.u_of(11, 0, (1 << 32) + 5) != u[5]
    # one value worked by hand from DESIGN.md 6 with Python integers
    def f(h):
        h &= 0xFFFFFFFF
        h ^= h >> 16
        h = h * 0x85EBCA6B & 0xFFFFFFFF
        h ^= h >> 13
        h = h * 0xC2B2AE35 & 0xFFFFFFFF
        return h ^ h >> 16
    seed, call, jj = (7 << 32) | 0xDEADBEEF, 3, 1234
    key = (f((seed & 0xFFFFFFFF) ^ 0x9E3779B9) + (seed >> 32) * 0x85EBCA77 + call * 0xC2B2AE3D) & 0xFFFFFFFF
    h1 = f(key + jj * 0x27D4EB2F)
    h2 = f(h1 ^ 0x68E31DA4 ^ key)
    assert X.u_of(seed, call, jj) == ((h1 >> 5) * (1 << 26) + (h2 >> 6)) / float(1 << 53)


def _check_against_float64(tree, op, res, ctx):
    """A model draw inside _per_reference's bracket with its slack, never on a zero leaf; the rebuilt tree inside
    check_invariant's arithmetic."""
    idx, leaf, least, reached = res
    leaves = tree.leaves.astype(np.float64)
    if least is None:
        assert (idx == -1).all() and not leaf.any(), ctx
        return
    k = op["k"]
    u = X.u_of(op["seed"], tree.draws_copy, np.arange(k)) if op["u"] is None else op["u"]
    F = R.prefix(leaves)
    t = R.targets(k, u, F[-1])
    s = R.slack(tree.L, F[-1])
    assert (idx >= 0).all() and (idx < tree.capacity).all(), ctx
    assert (leaves[idx] > 0).all() and np.array_equal(tree.leaves[idx], leaf), ctx
    assert (F[idx] - s <= t).all() and (t <= F[idx + 1] + s).all(), ctx
    assert least == leaf.min() and (idx[1:] >= idx[:-1]).all(), ctx


def _check_invariant_arithmetic(tree, ctx):
    for l in range(1, tree.L + 1):
        want = tree.levels[l - 1].astype(np.float64).reshape(-1, 64).sum(1)
        got = tree.levels[l][:len(want)].astype(np.float64)
        assert (np.abs(got - want) <= 64 * R.EPS32 * want).all(), (ctx, l)
        assert not tree.levels[l][len(want):].any(), (ctx, l)
    assert not tree.levels[0][tree.capacity:].any(), ctx


@pytest.mark.parametrize("cap", X.CAPACITIES)
def test_scripted_sequence_against_the_float64_model(cap):
    ops = X.script(SEED, cap)
    assert 50 <= len(ops) <= 75, len(ops)
    tree = X.ExactTree(cap)
    held = np.zeros(cap, bool)
    for n, (op, res) in enumerate(X.replay(tree, ops)):
        ctx = f"capacity {cap} op {n} {op['op']}"
        if op["op"] == "draw":
            _check_against_float64(tree, op, res, ctx)
        else:
            _check_invariant_arithmetic(tree, ctx)
        if op["op"] == "push":
            for lo, hi in res:
                assert (tree.leaves[lo:hi] == X.from_bits(tree.top)).all(), ctx
                held[lo:hi] = True
        if op["op"] == "update":
            held[op["idx"][res]] = True
            # the generator's promise: the batch's largest error sits on an accepted index of its own
            e = np.abs(op["td"])
            top = int(np.nanargmax(np.where(res, e, -1)))
            assert res[top] and ((op["idx"] == op["idx"][top]).sum() == 1 or (e[res] == e[top]).all()), ctx
            assert ((e[res] >= 1e-3) & (e[res] <= 1e3)).all(), ctx
        assert np.array_equal(tree.leaves > 0, held), ctx                        # only a slot that was given a leaf has one
        assert X.from_bits(tree.top) >= max(1.0, tree.leaves.max()), ctx
    assert tree.seq == sum(op["op"] == "draw" for op in ops)                     # _SEQ: one per sample call, never reset
    assert tree.draws < tree.seq                                                 # _DRAWS was zeroed on the way


@pytest.mark.parametrize("cap", X.CAPACITIES)
def test_scripted_sequence_coverage(cap):
    ops = X.script(SEED, cap)
    again = X.script(SEED, cap)
    assert len(ops) == len(again) and all(a["op"] == b["op"] for a, b in zip(ops, again))
    assert all(np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["td"], b["td"], equal_nan=True) for a, b in zip(ops, again) if a["op"] == "update")
    seen = X.coverage(ops, cap)
    L = X.layout(cap)[0]
    assert seen["zero"] and seen["full"] and seen["bad_cursor"] and seen["root_clamp"] and seen["empty_draw"] and seen["null_u"] and seen["given_u"]
    assert {0, 1, 63, 64, 65, cap} <= seen["counts"] and max(seen["counts"]) > cap
    assert seen["alphas"] == {0.0, 0.6, 1.0} and 1 in seen["batch"] and max(seen["batch"]) >= min(4096, 2 * cap)
    assert seen["ks"] == {k for k in (1, 7, 256, 4096) if k <= cap}
    assert seen["rejects"]
    if cap > 1:
        assert seen["cut"] and seen["dup"]
        assert seen["wrap_two_l2"] == (cap > 4096) and seen["wrap_one_l2"] == (L >= 2 and cap <= 4096)
        assert seen["wrap_one_l1"] or cap > 64            # (a longer ring meets it too when a near-full push starts in node 0)
    if cap >= 4097:
        assert seen["tiny"]
    # the two clamps of the descent are dead on a consistent tree (rounding is monotone): not required, and not reached
    assert seen["inner_clamp"] == 0


def test_zeroing_the_draw_counter_restarts_the_sequence_and_nothing_else():
    tree = X.ExactTree(5000).build((10.0 ** np.random.default_rng(2).uniform(-1, 1, 5000)).astype(np.float32))
    a = [tree.draw(256, None, 5000, seed=9)[0] for _ in range(3)]
    assert (tree.draws, tree.seq, tree.draws_copy, tree.seq_copy) == (3, 3, 2, 2) and not np.array_equal(a[0], a[1])
    assert tree.min_words[0] < X.F32_INF_BITS and tree.min_words[1] == X.F32_INF_BITS      # call 2 used word 0 and reset word 1
    tree.zero_draws()
    b = [tree.draw(256, None, 5000, seed=9)[0] for _ in range(3)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (tree.draws, tree.seq) == (3, 6)
    assert tree.min_words[1] < X.F32_INF_BITS and tree.min_words[0] == X.F32_INF_BITS      # call 5 used word 1


def test_single_leaf_change_moves_ancestors_the_old_tolerance_lets_stand():
    leaves, slot = X.single_leaf_case()
    stale = X.ExactTree(len(leaves)).build(leaves)
    moved = leaves.copy()
    moved[slot] += np.float32(1e-3)
    fresh = X.ExactTree(len(leaves)).build(moved)
    node = slot
    differs = []
    for l in range(1, fresh.L + 1):
        node >>= 6
        differs.append(stale.levels[l][node] != fresh.levels[l][node])
        kids = fresh.levels[l - 1][node * 64:node * 64 + 64].astype(np.float64).sum()
        accepted = abs(float(stale.levels[l][node]) - kids) <= 64 * R.EPS32 * kids
        assert accepted == (l >= 2), l                    # the old check sees the stale parent and none of the levels above it
    assert differs[0] and differs[1]
