"""An EXACT numpy model of the prioritized-replay sum tree, written from include/generals_vec.h ("prioritized experience
replay") and DESIGN.md 4.9 and 6, not from the kernels.  Where _per_reference.py says what a draw may be in float64 with a
slack, this module says what every word of the tree and every drawn index IS: a node is the last term of the sequential
float32 prefix of its 64 children, and np.cumsum(x, dtype=np.float32) adds in that order.

What it cannot predict is `powf`: the leaves an update writes and the weights stay under the measured tolerances of
test_prioritized_replay.py.  `update` therefore takes the leaves read back from the device and rebuilds what is above them.

The scripted operation sequences of tests/test_hip_per_exact.py are generated here (`script`) from a seed and a capacity
alone, and `coverage` says what a sequence reaches, so tests/test_per_exact_model.py asserts the coverage without a GPU."""
import numpy as np

from _policy_reference import M32, fmix32

HEADER_WORDS, HDR_MAX, HDR_REJECTED, HDR_DRAWS, HDR_MIN0, HDR_SEQ = 64, 0, 1, 2, 4, 6
F32_INF_BITS = 0x7F800000
U_TOP = 1.0 - 2.0 ** -53                     # the largest u: a draw's u is clamped into [0, U_TOP]
CAPACITIES = (1, 60, 64, 65, 100, 4097, 5000, 262145)


def bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)[()]


def layout(capacity):
    """(levels above the leaves, size in words, [first word of level 0 .. L]): a 64-word header, every level padded to a
    multiple of 64, the root level one node and its padding."""
    n, at = int(capacity), HEADER_WORDS
    off = [at]
    while True:
        at += (n + 63) // 64 * 64
        n = (n + 63) // 64
        off.append(at)
        if n <= 1:
            break
    return len(off) - 1, at + 64, off


def node_sums(children):
    """The level above `children` (float32, a multiple of 64 long): per 64 the last term of the left-to-right float32 prefix."""
    c = np.ascontiguousarray(children, np.float32).reshape(-1, 64)
    return np.cumsum(c, axis=1, dtype=np.float32)[:, 63].copy()


def _padded(values, words):
    out = np.zeros(words, np.float32)
    out[:len(values)] = values
    return out


def u_of(seed, call, j):
    """The 53-bit uniform of the u == NULL path for draw(s) j of the call whose _DRAWS word is `call`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    key = (fmix32(lo ^ np.uint64(0x9E3779B9)) + ((hi * np.uint64(0x85EBCA77)) & M32) + ((np.uint64(int(call) & 0xFFFFFFFF) * np.uint64(0xC2B2AE3D)) & M32)) & M32
    j = np.asarray(j, np.int64).astype(np.uint64)
    jlo, jhi = j & M32, j >> np.uint64(32)
    h1 = fmix32((key + jlo * np.uint64(0x27D4EB2F) + jhi * np.uint64(0x165667B1)) & M32)
    h2 = fmix32(h1 ^ np.uint64(0x68E31DA4) ^ key)
    return ((h1 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (h2 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


class ExactTree:
    """The tree of one ring: `levels[l]` float32, padded; the header words as Python ints."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.L, self.words, self.off = layout(capacity)
        self.widths = [(self.off[l + 1] if l < self.L else self.words) - self.off[l] for l in range(self.L + 1)]
        self.levels = [np.zeros(w, np.float32) for w in self.widths]
        self.top = bits(1.0)                 # gvec_per_init: all leaves 0, maximum 1.0, counters 0
        self.rejected = self.draws = self.seq = self.draws_copy = self.seq_copy = 0
        self.min_words = [F32_INF_BITS, F32_INF_BITS]

    # ---- the tree ----
    @property
    def leaves(self):
        return self.levels[0][:self.capacity]

    @property
    def total(self):
        return self.levels[self.L][0]

    def build(self, leaves32):
        """Every level above the given leaves, a short last node padded with zeros."""
        leaves32 = np.asarray(leaves32, np.float32)
        assert leaves32.shape == (self.capacity,)
        self.levels[0] = _padded(leaves32, self.widths[0])
        for l in range(1, self.L + 1):
            self.levels[l] = _padded(node_sums(self.levels[l - 1]), self.widths[l])
        return self

    def header(self):
        """The header's eight defined words as the device holds them."""
        return {HDR_MAX: self.top, HDR_REJECTED: self.rejected & 0xFFFFFFFF, HDR_DRAWS: self.draws & 0xFFFFFFFF, HDR_DRAWS + 1: self.draws_copy & 0xFFFFFFFF,
                HDR_MIN0: self.min_words[0], HDR_MIN0 + 1: self.min_words[1], HDR_SEQ: self.seq & 0xFFFFFFFF, HDR_SEQ + 1: self.seq_copy & 0xFFFFFFFF}

    def image(self):
        """The whole tree as uint32 words (header words the text does not define are 0)."""
        out = np.zeros(self.words, np.uint32)
        for w, v in self.header().items():
            out[w] = v
        for l in range(self.L + 1):
            out[self.off[l]:self.off[l] + self.widths[l]] = self.levels[l].view(np.uint32)
        return out

    # ---- gvec_per_push ----
    def push_runs(self, before, after, max_count):
        """(count, [(lo, hi), ...] the slot runs, cut): the rows between the two counter copies, clamped to the capacity and
        then to max_count; no run when the count is <= 0 or before's cursor is not inside the ring."""
        count = min(int(after[2]) - int(before[2]), self.capacity)
        cut = count > max_count
        count = min(count, int(max_count))
        cursor = int(before[0])
        if count <= 0 or not 0 <= cursor < self.capacity:
            return 0, [], cut
        first = min(cursor + count, self.capacity)
        runs = [(cursor, first)]
        if cursor + count > first:
            runs.append((0, cursor + count - first))
        return count, runs, cut

    def push(self, before, after, max_count):
        count, runs, cut = self.push_runs(before, after, max_count)
        self.rejected += int(cut)
        if runs:
            leaves = self.leaves.copy()
            for lo, hi in runs:
                leaves[lo:hi] = from_bits(self.top)
            self.build(leaves)
        return runs

    # ---- gvec_per_update ----
    def update_accepts(self, idx, td, alpha, eps):
        """Which (index, error) pairs are taken: the index inside the ring, the error finite, the value not overflowing."""
        idx, e = np.asarray(idx, np.int64), np.abs(np.asarray(td, np.float32))
        with np.errstate(all="ignore"):
            v = ((e + np.float32(eps)).astype(np.float64) ** float(alpha)).astype(np.float32)
        return (idx >= 0) & (idx < self.capacity) & np.isfinite(e) & np.isfinite(v) & (v >= 0)

    def update(self, idx, td, alpha, eps, leaves_after):
        """`leaves_after`: the leaves read back from the device (powf is not exact).  The maximum moves as bits to the largest
        accepted leaf: with duplicates a value that lost may have moved it too, so a caller who wants this exact gives the
        batch's largest error to one index only (`script` does)."""
        ok = self.update_accepts(idx, td, alpha, eps)
        self.rejected += int((~ok).sum())
        leaves_after = np.asarray(leaves_after, np.float32)
        taken = np.unique(np.asarray(idx, np.int64)[ok])
        if len(taken):
            self.top = max(self.top, int(leaves_after[taken].view(np.uint32).max()))
        self.build(leaves_after)
        return ok

    # ---- gvec_per_sample ----
    def zero_draws(self):
        """A caller zeroes _DRAWS and the word after it: the seed's sequence restarts, nothing else moves."""
        self.draws = self.draws_copy = 0

    def draw(self, k, u, size, seed=0):
        """(indices int64 [k], the drawn leaves float32 [k], the batch's smallest drawn leaf or None, reached): one
        gvec_per_sample call with `size` the ring's size word; u None: the counter RNG under `seed`.  `reached` counts the
        draws that took the root clamp and the two clamps of the descent."""
        k = int(k)
        call, seq = self.draws, self.seq
        self.draws_copy, self.seq_copy = call, seq
        self.min_words[(seq + 1) & 1] = F32_INF_BITS
        self.draws, self.seq = (call + 1) & 0xFFFFFFFF, (seq + 1) & 0xFFFFFFFF
        reached = {"root": 0, "inner": 0, "inner_zero": 0}
        total = self.total
        if size <= 0 or not total > 0:
            return np.full(k, -1, np.int64), np.zeros(k, np.float32), None, reached
        j = np.arange(k, dtype=np.int64)
        u = u_of(seed, call, j) if u is None else np.asarray(u, np.float64)
        u = np.where(u < 0.0, 0.0, np.where(u < 1.0, u, U_TOP))
        r = ((j.astype(np.float64) + u) / np.float64(k) * np.float64(total)).astype(np.float32)
        over = r >= total
        reached["root"] = int(over.sum())
        r = np.where(over, np.nextafter(total, np.float32(0)), r).astype(np.float32)
        node = np.zeros(k, np.int64)
        leaf = np.zeros(k, np.float32)
        rows = np.arange(k)
        for l in range(self.L, 0, -1):
            c = self.levels[l - 1].reshape(-1, 64)[node]
            P = np.cumsum(c, axis=1, dtype=np.float32)
            child = np.minimum((P <= r[:, None]).sum(1), 63)
            below = np.where(child > 0, P[rows, np.maximum(child - 1, 0)], np.float32(0)).astype(np.float32)
            leaf = c[rows, child]
            r = (r - below).astype(np.float32)
            clamp = r >= leaf
            reached["inner"] += int((clamp & (leaf > 0)).sum())
            reached["inner_zero"] += int((clamp & ~(leaf > 0)).sum())
            r = np.where(clamp, np.where(leaf > 0, np.nextafter(leaf, np.float32(0)), np.float32(0)), r).astype(np.float32)
            node = node * 64 + child
        least = int(leaf.view(np.uint32).min())
        self.min_words[seq & 1] = min(self.min_words[seq & 1], least)
        return node, leaf, from_bits(self.min_words[seq & 1]), reached


def weights(leaf, least, beta):
    """(leaf / the batch's smallest drawn leaf) ** -beta in float64; 0 where nothing was drawn."""
    leaf = np.asarray(leaf, np.float64)
    if least is None:
        return np.zeros(len(leaf))
    return (leaf / np.float64(least)) ** -float(beta)


def predicted_leaves(tree, idx, td, alpha, eps):
    """A stand-in for the device's leaves after an update, for runs without one: float64 pow rounded to float32, the LAST
    of duplicate indices winning."""
    ok = tree.update_accepts(idx, td, alpha, eps)
    out = tree.leaves.copy()
    v = ((np.abs(np.asarray(td, np.float32)) + np.float32(eps)).astype(np.float64)[ok] ** float(alpha)).astype(np.float32)
    out[np.asarray(idx, np.int64)[ok]] = v
    return out


def single_leaf_case():
    """Leaves near 1 on the four-level ring, and the slot whose leaf the single-leaf tests move by 1e-3."""
    rng = np.random.default_rng(77)
    leaves = (0.9 + 0.2 * rng.random(262145)).astype(np.float32)
    return leaves, 131072 + 4096 + 64 + 3


# ---- the scripted sequences -------------------------------------------------------------------------------------------
def script(seed, capacity):
    """About 60 operations for one ring, from the seed and the capacity alone.  Each is a dict: op "push" (before, after,
    max_count), "update" (idx, td, alpha, eps), "draw" (k, u or None, seed, beta, counters), "zero_draws".  The ring's
    counters move as a ring's would, except where an operation says otherwise (a bad cursor, an empty ring)."""
    rng = np.random.default_rng([int(seed), int(capacity)])
    cap = int(capacity)
    ops = []
    ring = [0, 0, 0, 0]                                   # cursor, size, total pushed, 0
    eps = 1e-6

    def push(count, max_count=None, cursor=None, bad=False):
        before = list(ring)
        if cursor is not None:
            before[0] = int(cursor)
        after = list(before)
        if not bad:
            after[0] = (before[0] + count) % cap
        after[1] = min(before[1] + count, cap)
        after[2] = before[2] + count
        ops.append(dict(op="push", before=before, after=after, max_count=int(max_count if max_count is not None else max(count, 1))))
        if not bad:
            ring[:] = after

    def update(n, alpha, dup=False, rejects=False, lo=-3.0, hi=3.0):
        idx = rng.integers(0, cap, n)
        td = (10.0 ** rng.uniform(lo, hi - 0.5, n)).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
        if dup and n >= 4:
            idx[1:n // 2] = idx[0]                        # one slot many times, other values
            idx[n // 2] = idx[n - 1]
        if rejects and n >= 8:
            idx[2], idx[3] = -1, cap
            td[4], td[5], td[6] = np.nan, np.inf, -np.inf
            idx[7] = cap + (1 << 40)
        # the batch's largest error sits on an index of its own: the maximum it leaves is then readable from the leaves
        top = int(rng.integers(0, n))
        if rejects and n >= 8 and top in (2, 3, 4, 5, 6, 7):
            top = 0
        td[top] = np.float32(10.0 ** hi * 0.999)
        others = np.arange(n) != top
        if cap > 1:
            idx[others & (idx == idx[top])] = (idx[top] + 1) % cap            # the others give way (and stay duplicates of each other)
        else:
            td[others & np.isfinite(td)] = td[top]        # one slot: every value the same
        ops.append(dict(op="update", idx=idx.astype(np.int64), td=td, alpha=float(alpha), eps=eps))

    def draw(k, given, beta=0.4, rseed=0, counters=None, u=None):
        if given and u is None:
            u = rng.random(k)
        ops.append(dict(op="draw", k=int(k), u=u, seed=int(rseed), beta=float(beta), counters=list(counters if counters is not None else ring)))

    ks = [k for k in (1, 7, 256, 4096) if k <= max(cap, 1) or k == 1]
    draw(1, True)                                         # an empty ring and an empty tree
    draw(ks[-1], True, counters=[0, 5, 5, 0])             # a ring that says it holds rows over an empty tree
    update(min(cap, 8), 0.6)                              # leaves without rows: the tree is not empty, the ring is
    draw(ks[-1], False, rseed=3)
    draw(1, True, counters=[0, 0, 0, 0])
    # fill the ring, in pieces of every interesting length, to its end and round it
    for count in (0, 1, 63, 64, 65):
        push(count)
        draw(int(rng.choice(ks)), bool(rng.integers(2)), beta=float(rng.choice([0.0, 0.4, 1.0])), rseed=5)
    update(int(rng.integers(1, 4097)), 0.6, dup=True)
    push(max(cap - ring[0] - 1, 0))                       # the cursor goes to the last slot
    push(2)                                               # the smallest wrap: one slot at each end
    push(cap)                                             # exactly the ring
    push(cap + 77)                                        # more than the ring
    update(min(cap * 2, 4096), 1.0, dup=True, rejects=True)
    draw(ks[-1], True, u=np.linspace(0.0, 1.0, ks[-1], endpoint=False))
    draw(ks[-1], True, u=np.full(ks[-1], U_TOP))          # the last draw takes the root clamp
    draw(ks[-1], True, u=np.zeros(ks[-1]))
    # wrapping pushes from cursors near the ring's end, some cut short
    for i in range(6):
        tail = int(rng.integers(1, min(cap, 70) + 1)) if cap > 1 else 1
        head = int(rng.integers(1, min(cap, 130) + 1))
        count = min(tail + head, cap)
        cursor = (cap - tail) % cap
        if i % 3 == 2 and count > 1:
            push(count, max_count=int(rng.integers(1, count)), cursor=cursor)
        else:
            push(count, cursor=cursor)
        update(int(rng.integers(1, 4097)), float(rng.choice([0.0, 0.6, 1.0])), dup=bool(i & 1), rejects=(i == 3))
        draw(int(rng.choice(ks)), bool(i & 1), beta=float(rng.choice([0.0, 0.4, 1.0])), rseed=11 + i)
    push(5, cursor=cap, bad=True)                         # a cursor that is not inside the ring: once above,
    push(min(cap, 64), max_count=64, cursor=-1, bad=True)  # once below
    push(cap, max_count=max(cap // 2, 1), cursor=ring[0])  # a whole ring of rows, half of them let in
    # every leaf near 1, then one leaf moved by very little: the upper levels must follow
    update_all = np.arange(cap, dtype=np.int64)
    ops.append(dict(op="update", idx=update_all, td=(0.9 + 0.2 * rng.random(cap)).astype(np.float32), alpha=1.0, eps=eps))
    last = ops[-1]
    last["td"][int(rng.integers(0, cap))] = np.float32(1.25)          # the batch's one largest error
    one = int(rng.integers(0, cap))
    ops.append(dict(op="update", idx=np.array([one], np.int64), td=np.array([last["td"][one] + np.float32(1e-3)], np.float32), alpha=1.0, eps=eps))
    draw(ks[-1], False, rseed=99)
    ops.append(dict(op="zero_draws"))                     # the seed's sequence restarts: the same indices again
    draw(ks[-1], False, rseed=99)
    for k in ks:
        draw(k, False, beta=1.0, rseed=(1 << 40) + 7)
        draw(k, True, beta=0.4)
    push(1)
    update(1, 0.6)
    draw(1, True)
    return ops


def replay(tree, ops, leaves_after_update=None):
    """Runs `ops` on the model, the leaves after an update from `leaves_after_update(tree, op)` (default: predicted); yields
    (op, result) after each."""
    for op in ops:
        if op["op"] == "push":
            res = tree.push(op["before"], op["after"], op["max_count"])
        elif op["op"] == "update":
            leaves = (leaves_after_update or (lambda t, o: predicted_leaves(t, o["idx"], o["td"], o["alpha"], o["eps"])))(tree, op)
            res = tree.update(op["idx"], op["td"], op["alpha"], op["eps"], leaves)
        elif op["op"] == "draw":
            res = tree.draw(op["k"], op["u"], op["counters"][1], op["seed"])
        else:
            res = tree.zero_draws()
        yield op, res


def coverage(ops, capacity):
    """What a sequence reaches, found by replaying it on the model (nothing here trusts the generator's intentions)."""
    tree = ExactTree(capacity)
    seen = dict(wrap_two_l2=False, wrap_one_l2=False, wrap_one_l1=False, full=False, zero=False, cut=False, bad_cursor=False, dup=False, rejects=False,
                tiny=False, root_clamp=False, inner_clamp=0, empty_draw=False, null_u=False, given_u=False, counts=set(), ks=set(), alphas=set(), batch=set())
    for op in ops:
        if op["op"] == "push":
            raw = op["after"][2] - op["before"][2]
            count, runs, cut = tree.push_runs(op["before"], op["after"], op["max_count"])
            seen["counts"].add(raw)
            seen["zero"] |= raw == 0
            seen["full"] |= raw >= capacity and bool(runs) and not cut
            seen["cut"] |= cut and bool(runs)
            seen["bad_cursor"] |= raw > 0 and not 0 <= op["before"][0] < capacity
            if len(runs) == 2:
                a, b = (runs[0][1] - 1), (runs[1][1] - 1)
                if tree.L >= 2:
                    seen["wrap_two_l2" if a >> 12 != b >> 12 else "wrap_one_l2"] = True
                seen["wrap_one_l1"] |= (runs[0][0] >> 6) == (b >> 6)
        elif op["op"] == "update":
            ok = tree.update_accepts(op["idx"], op["td"], op["alpha"], op["eps"])
            good = op["idx"][ok]
            seen["dup"] |= len(np.unique(good)) < len(good)
            seen["rejects"] |= bool((~ok).any())
            seen["alphas"].add(op["alpha"])
            seen["batch"].add(len(op["idx"]))
            if len(op["idx"]) == 1 and ok.all():
                new = predicted_leaves(tree, op["idx"], op["td"], op["alpha"], op["eps"])[op["idx"][0]]
                delta = abs(float(new) - float(tree.leaves[op["idx"][0]]))
                seen["tiny"] |= 0 < delta < 1e-6 * float(tree.total)
        elif op["op"] == "draw":
            seen["ks"].add(op["k"])
            seen["null_u" if op["u"] is None else "given_u"] = True
        for _, res in replay(tree, [op]):
            if op["op"] == "draw":
                seen["root_clamp"] |= res[3]["root"] > 0
                seen["inner_clamp"] += res[3]["inner"] + res[3]["inner_zero"]
                seen["empty_draw"] |= res[2] is None
    return seen
