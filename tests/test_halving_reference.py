"""The numpy restatement of the sequential-halving search (tests/_halving_reference.py) against what already exists - the
playout score, the counter hash, the schedule of the Python front - and against its own definition.  CPU only."""
import types

import numpy as np
import pytest
import torch

import _halving_reference as HR


def _engine(W=3, H=2):
    """what the Python front reads of an engine; nothing here calls the library"""
    return types.SimpleNamespace(max_w=W, max_h=H, max_p=2, B=4, device=0)


@pytest.mark.parametrize("w", [dict(), dict(win=2.0, loss=-3.0, land=0.25, army=1.5)], ids=["default", "weighted"])
def test_scores_equal_playout_score_bit_for_bit(w):
    from generalsreinforcementlearning_amd import PlayoutScore
    t = HR.random_terms(np.random.default_rng(3), (50, 7, 3))
    kinds = (t[..., 3] == 1).any(), ((t[..., 0] == 1) & (t[..., 2] == 0)).any(), (t[..., 0] == 0).any(), \
        ((t[..., 0] == 1) & (t[..., 4] + t[..., 6] == 0)).any()
    assert all(kinds)
    want = PlayoutScore(**w)(torch.from_numpy(t)).numpy()
    got = HR.playout_scores(t, **w)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("m,budget,rounds,spent", [(1, 64, [(1, 64)], 64), (2, 64, [(2, 32)], 64), (3, 64, [(3, 10), (2, 16)], 62),
                                                   (5, 64, [(5, 4), (3, 7), (2, 10)], 61), (16, 64, [(16, 1), (8, 2), (4, 4), (2, 8)], 64),
                                                   (33, 64, None, 33 + 17 + 9 + 5 * 2 + 3 * 3 + 2 * 5),
                                                   (64, 64, None, 64 + 32 + 16 + 8 * 1 + 4 * 2 + 2 * 5), (64, 256, None, None)])
def test_schedules_end_at_one(m, budget, rounds, spent):
    from generalsreinforcementlearning_amd import HalvingSearch, halving_schedule
    s = HR.schedule(m, budget)
    assert s == halving_schedule(m, budget)
    if rounds is not None:
        assert s == rounds
    assert s[0][0] == m and -(-s[-1][0] // 2) == 1 and all(-(-a[0] // 2) == b[0] for a, b in zip(s, s[1:]))
    T = len(s)
    assert T == max(1, int(np.ceil(np.log2(m)))) and all(R == max(1, budget // (T * K)) for K, R in s)
    front = HalvingSearch(_engine(), candidates=m, budget=budget, depth=2)
    assert front.schedule == s and front.playouts_per_row == HR.playouts_per_row(m, budget) == sum(K * R for K, R in s)
    if spent is not None:
        assert front.playouts_per_row == spent


def _one_playout(score_half):
    """a valid playout row whose default score is score_half / 100 - 0.5: land 50 %, army score_half %"""
    return [1, 4, 1, 0, 10, score_half, 10, 100 - score_half]


def test_ties_go_to_the_lower_slot_and_empty_slots_rank_last():
    # four columns: slots 0 and 2 tie, slot 1 has no valid playout, slot 3 is worse
    terms = np.array([[[_one_playout(60)], [[0] * 8], [_one_playout(60)], [_one_playout(20)]]], np.int32)
    cand0 = np.array([[11, 12, 13, 14]], np.int64)
    prior = np.zeros((1, 4))
    total, count = np.zeros((1, 4)), np.zeros((1, 4), np.int32)
    slot, cand = HR.halve(terms, None, cand0, prior, total, count, 4)
    assert slot.tolist() == [[0, 2, 3, 1]] and cand.tolist() == [[11, 13, 14, 12]]
    assert count.tolist() == [[1, 0, 1, 1]] and total[0, 0] == total[0, 2] == 0.5 * 0.5 + 0.5 * 0.6 - 0.5
    # a prior that prefers the empty slot does not help it; one that prefers slot 3 by enough does
    prior = np.array([[0.0, 100.0, 0.0, 10.0]])                  # the gap in sigma is (50 + 1) * (0.05 - -0.15) / 2 = 5.1
    total[:], count[:] = 0, 0
    slot, _ = HR.halve(terms, None, cand0, prior, total, count, 2)
    assert slot.tolist() == [[3, 0]]
    # padding ranks last even with a count
    total[:], count[:] = 0, 0
    slot, cand = HR.halve(terms, None, np.array([[HR.NONE, 12, 13, 14]], np.int64), np.zeros((1, 4)), total, count, 4)
    assert slot.tolist() == [[2, 3, 0, 1]] and cand[0, 2] == HR.NONE


def test_two_rounds_through_a_permuted_slot_equal_one_pass():
    rng = np.random.default_rng(5)
    n, m = 6, 8
    cand0 = np.arange(n * m, dtype=np.int64).reshape(n, m)
    prior = rng.normal(size=(n, m))
    t0, t1 = HR.random_terms(rng, (n, m, 2)), HR.random_terms(rng, (n, 4, 3))
    total, count = np.zeros((n, m)), np.zeros((n, m), np.int32)
    slot, cand = HR.halve(t0, None, cand0, prior, total, count, 4)
    assert (np.sort(slot, axis=1) != np.arange(4)).any()                     # not the identity
    assert all(cand[r].tolist() == cand0[r, slot[r]].tolist() for r in range(n))
    slot2, _ = HR.halve(t1, slot, cand0, prior, total, count, 2)
    # one pass: every slot's playouts of both rounds, concatenated in order
    scores0, scores1 = HR.playout_scores(t0), HR.playout_scores(t1)
    for r in range(n):
        for s in range(m):
            rows = [(t0[r, s, j], scores0[r, s, j]) for j in range(2)]
            where = np.flatnonzero(slot[r] == s)
            if len(where):
                rows += [(t1[r, where[0], j], scores1[r, where[0], j]) for j in range(3)]
            acc, cnt = 0.0, 0
            for t, v in rows:
                if t[0]:
                    acc, cnt = acc + float(v), cnt + 1
            assert total[r, s] == acc and count[r, s] == cnt
        assert set(slot2[r].tolist()) <= set(slot[r].tolist())


def test_gumbel_keys_follow_the_counter_hash():
    from generalsreinforcementlearning_amd import HalvingSearch
    from generalsreinforcementlearning_amd.search import _uniform_keys
    seed, n, A = (7 << 32) + 12345, 5, 30
    u = _uniform_keys(seed, n, A, torch.device("cpu")).numpy()
    h = np.array([[HR.hash32(seed, r, a) for a in range(A)] for r in range(n)], np.float64)
    assert np.array_equal(u * 4294967296.0, h)
    s = HalvingSearch(_engine(), candidates=4, budget=8, depth=2)
    mask = torch.zeros(n, A, dtype=torch.bool)
    mask[0, [2, 5, 9, 14, 20, 21]] = True
    mask[1, [3, 8]] = True
    mask[3, :] = True
    mask[4, 7] = True
    logits = torch.from_numpy(np.random.default_rng(1).normal(size=(n, A)).astype(np.float32))
    for lg in (None, logits):
        cand, prior = s.propose(mask, lg, seed)
        wc, wp = HR.propose(mask.numpy(), None if lg is None else lg.numpy(), seed, 4)
        assert cand.dtype == torch.int64 and prior.dtype == torch.float64 and cand.is_contiguous() and prior.is_contiguous()
        assert np.array_equal(cand.numpy(), wc)
        live = wc != HR.NONE
        assert np.allclose(prior.numpy()[live], wp[live], rtol=1e-14, atol=1e-14) and np.isneginf(prior.numpy()[~live]).all()
    assert cand[1].tolist()[2:] == [HR.NONE] * 2 and cand[2].tolist() == [HR.NONE] * 4 and cand[4].tolist() == [7] + [HR.NONE] * 3


# ---- the improved policy --------------------------------------------------------------------------------------------------
def _policy_case():
    rng = np.random.default_rng(9)
    n, A, m = 5, 30, 4
    logits = rng.normal(size=(n, A))
    mask = rng.random((n, A)) < 0.5
    mask[1] = False                                              # a dead row
    mask[2, [3, 7, 11]] = True
    cand = np.stack([rng.permutation(A)[:m] for _ in range(n)]).astype(np.int64)
    cand[2] = [3, 7, HR.PASS, HR.NONE]
    count = rng.integers(1, 5, (n, m)).astype(np.int32)
    count[3] = 0                                                 # nothing visited
    total = rng.uniform(-1, 1, (n, m)) * count
    return logits, mask, cand, total, count


def test_the_target_is_a_distribution_on_the_legal_set():
    logits, mask, cand, total, count = _policy_case()
    target, v_mix = HR.improved_policy(logits, mask, cand, total, count)
    live = mask.any(1)
    assert np.abs(target[live].sum(1) - 1).max() < 1e-12 and (target[~live] == 0).all() and (target[~mask] == 0).all()
    assert (target[mask] > 0).all()
    # nothing visited: the prior, and v_mix is the value (or 0)
    e = np.where(mask[3], np.exp(logits[3] - logits[3][mask[3]].max()), 0.0)
    assert np.allclose(target[3], e / e.sum(), rtol=1e-14, atol=0) and v_mix[3] == 0.0 and v_mix[1] == 0.0
    value = np.linspace(-0.5, 0.5, 5)
    t2, v2 = HR.improved_policy(logits, mask, cand, total, count, value)
    assert v2[3] == value[3] and v2[1] == value[1] and np.array_equal(t2[3], target[3])


def test_v_mix_follows_the_formula_and_the_target_grows_in_q():
    logits, mask, cand, total, count = _policy_case()
    r = 2                                                        # V = {3, 7}: the pass and the padding are ignored
    x = logits[r]
    pi = np.where(mask[r], np.exp(x - x[mask[r]].max()), 0.0)
    pi /= pi.sum()
    q = total[r, :2] / count[r, :2]
    vq = (pi[[3, 7]] * q).sum() / pi[[3, 7]].sum()
    _, v = HR.improved_policy(logits, mask, cand, total, count)
    assert abs(v[r] - vq) < 1e-14
    value = np.full(5, 0.3)
    _, v = HR.improved_policy(logits, mask, cand, total, count, value)
    N = count[r, :2].sum()
    assert abs(v[r] - (0.3 + N * vq) / (1 + N)) < 1e-14
    # a visited action's probability grows with its q, everything else equal
    base, _ = HR.improved_policy(logits, mask, cand, total, count, value)
    better = total.copy()
    better[r, 0] += 0.2 * count[r, 0]
    more, _ = HR.improved_policy(logits, mask, cand, better, count, value)
    assert more[r, 3] > base[r, 3]
    # a candidate outside the mask is not visited
    mask2 = mask.copy()
    mask2[r, 7] = False
    _, v = HR.improved_policy(logits, mask2, cand, total, count)
    assert abs(v[r] - q[0]) < 1e-14
