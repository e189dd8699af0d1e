"""TEST INFRASTRUCTURE - the sequential-halving search restated in numpy and plain Python (include/generals_vec.h
"sequential-halving search"): the schedule, the playout score, a round's accumulate-and-select with
loops in the stated order, the Gumbel keys in exact integer arithmetic plus float64, and the improved policy in float64.
Nothing here imports the package: tests/test_halving_reference.py ties it to PlayoutScore and to its own definition, the GPU
tests hold the kernels to it."""
import math

import numpy as np

PASS, NONE = -1, -2                      # GVEC_SEARCH_PASS, GVEC_SEARCH_NONE
DEFAULT_WEIGHTS = dict(win=1.0, loss=-1.0, land=0.5, army=0.5)
M64 = 2 ** 64 - 1


# ---- synthetic playout terms ------------------------------------------------------------------------------------------------
def random_terms(rng, shape):
    """int32 [*shape, 8] with won, dead, zero-denominator and invalid rows among ordinary ones"""
    t = np.zeros(tuple(shape) + (8,), np.int32)
    t[..., 0] = 1
    t[..., 1] = rng.integers(1, 9, shape)
    t[..., 2] = 1
    t[..., 4:8] = rng.integers(0, 400, tuple(shape) + (4,))
    kind = rng.integers(0, 8, shape)
    t[kind == 0, 3] = 1                                          # won
    t[kind == 1, 2] = 0                                          # dead
    t[kind == 2, 4] = t[kind == 2, 6] = 0                        # land denominators zero
    t[kind == 3, 4:8] = 0                                        # both zero
    t[kind == 4] = 0                                             # invalid: all zeros
    return t


# ---- the schedule -----------------------------------------------------------------------------------------------------------
def schedule(m, budget):
    """[(K_r, R_r)]: K_0 = m, K_{r+1} = ceil(K_r / 2), T = max(1, ceil(log2 m)) rounds, R_r = max(1, budget // (T * K_r))"""
    T = max(1, math.ceil(math.log2(m))) if m > 1 else 1
    out, K = [], m
    for _ in range(T):
        out.append((K, max(1, budget // (T * K))))
        K = -(-K // 2)
    return out


def playouts_per_row(m, budget):
    return sum(K * R for K, R in schedule(m, budget))


def round_seed(seed, r):
    return ((seed & M64) + (r + 1) * 0x9E3779B97F4A7C15) & M64


def q_range(win=1.0, loss=-1.0, land=0.5, army=0.5):
    """(q_lo, q_inv_range): the playout value on [0, 1]"""
    lo = min(loss, -(land + army) / 2)
    return lo, 1.0 / (max(win, (land + army) / 2) - lo)


# ---- the score of one playout (PlayoutScore.__call__, operation for operation, float64) -----------------------------------------
def playout_scores(terms, win=1.0, loss=-1.0, land=0.5, army=0.5):
    t = np.asarray(terms).astype(np.float64)

    def ratio(mine, others):
        den = mine + others
        return np.where(den != 0, mine / np.where(den != 0, den, 1.0), 0.5)

    shaped = (land * ratio(t[..., 4], t[..., 6]) + army * ratio(t[..., 5], t[..., 7])) - (land + army) / 2
    out = np.where(t[..., 2] == 0, loss, shaped)
    return np.where(t[..., 3] != 0, win, out)


# ---- one round: accumulate, then select -------------------------------------------------------------------------------------
def halve(terms, slot, candidates0, prior_key, total, count, k_next, weights=None, c_visit=50.0, c_scale=1.0):
    """terms int32 [n, k, R, 8], slot int [n, k] or None (the identity), candidates0 int64 [n, m], prior_key float64 [n, m];
    total float64 [n, m] and count int32 [n, m] are updated in place -> (next_slot int32 [n, k_next], next_candidates int64
    [n, k_next])"""
    w = dict(DEFAULT_WEIGHTS, **(weights or {}))
    q_lo, q_inv = q_range(**w)
    terms = np.asarray(terms)
    n, k, R, _ = terms.shape
    m = candidates0.shape[1]
    assert slot is not None or k == m
    scores = playout_scores(terms, **w)
    next_slot = np.zeros((n, k_next), np.int32)
    next_cand = np.zeros((n, k_next), np.int64)
    for r in range(n):
        slots = [c if slot is None else int(slot[r, c]) for c in range(k)]
        for c, s in enumerate(slots):
            for j in range(R):                                   # in this order: the sum is a float64 chain
                if terms[r, c, j, 0] != 0:
                    total[r, s] = float(total[r, s]) + float(scores[r, c, j])
                    count[r, s] += 1
        nmax = int(count[r].max())
        order = []
        for s in slots:
            live = count[r, s] > 0 and candidates0[r, s] != NONE
            key = 0.0
            if live:
                mean = float(total[r, s]) / float(count[r, s])
                key = float(prior_key[r, s]) + ((c_visit + float(nmax)) * c_scale) * ((mean - q_lo) * q_inv)
            order.append((0 if live else 1, -key, s))            # live first, the larger key, the lower slot
        order.sort()
        for q in range(k_next):
            next_slot[r, q] = order[q][2]
            next_cand[r, q] = candidates0[r, order[q][2]]
    return next_slot, next_cand


def search(play, candidates0, prior_key, budget, seed, weights=None, c_visit=50.0, c_scale=1.0):
    """the rounds, with play(candidates int64 [n, K], R, round, seed_of_the_round) -> terms [n, K, R, 8] supplying the
    playouts -> (total, count, slot [n], action [n])"""
    n, m = candidates0.shape
    total, count = np.zeros((n, m), np.float64), np.zeros((n, m), np.int32)
    cand, slot = candidates0, None
    for r, (K, R) in enumerate(schedule(m, budget)):
        terms = play(cand, R, r, round_seed(seed, r))
        slot, cand = halve(terms, slot, candidates0, prior_key, total, count, -(-K // 2), weights, c_visit, c_scale)
    return total, count, slot[:, 0], cand[:, 0]


# ---- Gumbel-top-m -----------------------------------------------------------------------------------------------------------
def hash32(seed, row, action):
    """_uniform_keys' counter hash of (seed, row, action), in Python integers"""
    M = 0xFFFFFFFF
    s = seed & M64
    x = ((s & M) ^ ((s >> 32) * 0x9E3779B1 & M)) + row * 0x85EBCA6B + action * 0xC2B2AE35
    for mul in (0x7FEB352D, 0x846CA68B):
        x &= M
        x ^= x >> 16
        x = (x * mul) & M
    x ^= x >> 15
    return x & M


def gumbel(seed, n, A):
    """float64 [n, A]: g = -log(-log u), u = (h + 0.5) / 2^32"""
    u = np.array([[(hash32(seed, r, a) + 0.5) / 4294967296.0 for a in range(A)] for r in range(n)], np.float64).reshape(n, A)
    return -np.log(-np.log(u))


def propose(mask, logits, seed, m):
    """(candidates int64 [n, m], prior_key float64 [n, m]): the m legal actions with the largest logit + g, in that order
    (the lower index among equals), padded with NONE / -inf"""
    mask = np.asarray(mask) != 0
    n, A = mask.shape
    keys = gumbel(seed, n, A) + (0.0 if logits is None else np.asarray(logits, np.float64))
    cand = np.full((n, m), NONE, np.int64)
    prior = np.full((n, m), -np.inf, np.float64)
    for r in range(n):
        legal = np.flatnonzero(mask[r])
        top = sorted(legal, key=lambda a: (-keys[r, a], a))[:m]
        cand[r, :len(top)] = top
        prior[r, :len(top)] = keys[r, top]
    return cand, prior


# ---- the improved policy, float64 -------------------------------------------------------------------------------------------
def _softmax_on(x, on):
    out = np.zeros_like(x)
    z = x[on]
    e = np.exp(z - z.max())
    out[on] = e / e.sum()
    return out


def improved_policy(logits, mask, candidates0, total, count, value=None, weights=None, c_visit=50.0, c_scale=1.0):
    """logits [n, A] or None, mask [n, A], candidates0 / total / count [n, m], value [n] or None -> (target float64 [n, A],
    v_mix float64 [n])"""
    w = dict(DEFAULT_WEIGHTS, **(weights or {}))
    q_lo, q_inv = q_range(**w)
    mask = np.asarray(mask) != 0
    n, A = mask.shape
    m = candidates0.shape[1]
    target, v_mix = np.zeros((n, A), np.float64), np.zeros(n, np.float64)
    for r in range(n):
        x = np.zeros(A) if logits is None else np.asarray(logits[r], np.float64)
        on = mask[r] & (x > -np.inf)
        v_mix[r] = 0.0 if value is None else float(value[r])
        if not on.any():
            continue
        pi = _softmax_on(x, on)
        V = [l for l in range(m) if count[r, l] > 0 and 0 <= candidates0[r, l] < A and on[candidates0[r, l]]]
        if not V:
            target[r] = pi
            continue
        a = np.array([candidates0[r, l] for l in V])
        q = np.array([float(total[r, l]) / float(count[r, l]) for l in V])
        N = float(sum(int(count[r, l]) for l in V))
        lw = x[a] - x[a].max()                                   # pi(a) / sum_V pi: the prior's normaliser cancels
        vq = float((np.exp(lw) * q).sum() / np.exp(lw).sum())
        v_mix[r] = vq if value is None else (float(value[r]) + N * vq) / (1.0 + N)
        completed = np.full(A, v_mix[r])
        completed[a] = q
        sigma = ((c_visit + float(count[r].max())) * c_scale) * ((completed - q_lo) * q_inv)
        target[r] = _softmax_on(np.where(on, x + sigma, -np.inf), on)
    return target, v_mix
