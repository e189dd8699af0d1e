"""The prioritized-replay kernels (gvec_per_*, PrioritizedDeviceReplayBuffer) against the exact model of
_per_exact.py: after every operation the whole tree is read back and every header word, every node above the leaves, the
padding and every drawn index must be the model's, bit for bit.  Only what `powf` makes - an update's leaves and the weights -
is held to the measured tolerances of test_prioritized_replay.py."""
import numpy as np
import pytest

import _per_exact as X
import _per_reference as R
from test_per_exact_model import SEED
from test_prioritized_replay import LEAF_TOL, WEIGHT_TOL

pytestmark = pytest.mark.gpu


class Device:
    """A tree on the device and the model beside it; every call compares the two."""

    def __init__(self, capacity, **kw):
        import torch
        from generalsreinforcementlearning_amd.env_pool import PrioritizedDeviceReplayBuffer
        self.t = torch
        self.buf = PrioritizedDeviceReplayBuffer(capacity, **kw).allocate((1,))
        self.model = X.ExactTree(capacity)
        self.cap = capacity
        self.same("init")

    def raw(self):
        return self.buf.tree.cpu().numpy().view(np.uint32)

    def leaves(self, raw):
        return raw[self.model.off[0]:self.model.off[0] + self.cap].view(np.float32)

    def same(self, ctx, raw=None):
        """The device's tree is the model's: header (the maximum as bits, _REJECTED, _DRAWS, _SEQ, their copies, the two
        minimum words, the unused words 0), every level, the padding."""
        raw = self.raw() if raw is None else raw
        want = self.model.image()
        assert raw.shape == want.shape, ctx
        assert np.array_equal(raw[:X.HEADER_WORDS], want[:X.HEADER_WORDS]), f"{ctx}: header {raw[:8]} != {want[:8]}"
        m = self.model
        for l in range(m.L + 1):
            got, exp = raw[m.off[l]:m.off[l] + m.widths[l]], want[m.off[l]:m.off[l] + m.widths[l]]
            bad = np.flatnonzero(got != exp)
            assert not len(bad), f"{ctx}: level {l}: {len(bad)} words differ, first {bad[:5]}: {got[bad[:5]].view(np.float32)} != {exp[bad[:5]].view(np.float32)}"

    def _dev(self, a, dtype):
        return self.t.as_tensor(np.asarray(a), dtype=dtype).to(self.buf.device)

    def push(self, before, after, max_count, ctx):
        t, b = self.t, self.buf
        bt, at = self._dev(before, t.int64), self._dev(after, t.int64)
        rc = b._L.gvec_per_push(b.device.index, b._stream(), b.tree.data_ptr(), self.cap, bt.data_ptr(), at.data_ptr(), int(max_count))
        assert rc == 0, ctx
        self.model.push(before, after, max_count)
        self.same(ctx)                                   # a push's leaves are the maximum: exact, like everything above them

    def check_update(self, idx, td, alpha, eps, ctx):
        """After the device's update: untouched leaves are the same bits, a touched one is within LEAF_TOL of a value supplied
        for it, and everything above the read-back leaves is the model's rebuild."""
        old = self.model.leaves.copy()
        raw = self.raw()
        new = self.leaves(raw).copy()
        ok = self.model.update(idx, td, alpha, eps, new)
        idx = np.asarray(idx, np.int64)
        touched = np.zeros(self.cap, bool)
        touched[idx[ok]] = True
        assert np.array_equal(new[~touched].view(np.uint32), old[~touched].view(np.uint32)), ctx
        want = R.leaf_value(np.asarray(td, np.float32)[ok], alpha, eps)
        near = np.abs(new[idx[ok]] - want) <= LEAF_TOL * want
        hit = np.zeros(self.cap, bool)
        np.logical_or.at(hit, idx[ok], near)
        assert np.array_equal(hit, touched), f"{ctx}: {int((touched & ~hit).sum())} leaves are none of their supplied values"
        self.same(ctx, raw)

    def update(self, idx, td, alpha, eps, ctx):
        t, b = self.t, self.buf
        it, tt = self._dev(idx, t.int64), self._dev(td, t.float32)
        rc = b._L.gvec_per_update(b.device.index, b._stream(), b.tree.data_ptr(), self.cap, it.data_ptr(), tt.data_ptr(), len(idx), alpha, eps)
        assert rc == 0, ctx
        self.check_update(idx, td, alpha, eps, ctx)

    def check_draw(self, got_idx, got_w, k, u, size, seed, beta, ctx):
        idx, leaf, least, _ = self.model.draw(k, u, size, seed)
        got_idx, got_w = got_idx.cpu().numpy(), got_w.cpu().numpy()
        bad = np.flatnonzero(got_idx != idx)
        assert not len(bad), f"{ctx}: {len(bad)} of {k} indices differ, first at {bad[:5]}: {got_idx[bad[:5]]} != {idx[bad[:5]]}"
        if least is None:
            assert (got_idx == -1).all() and (got_w == 0).all(), ctx
        else:
            want = X.weights(leaf, least, beta)
            assert (np.abs(got_w - want) <= WEIGHT_TOL * want).all(), ctx
            assert got_w.max() == 1.0, ctx
        self.same(ctx)

    def draw(self, k, u, counters, seed, beta, ctx):
        t, b = self.t, self.buf
        ct = self._dev(counters, t.int64)
        ut = None if u is None else self._dev(u, t.float64)
        idx = t.full((k,), -7, dtype=t.int64, device=b.device)
        w = t.full((k,), -7.0, dtype=t.float32, device=b.device)
        rc = b._L.gvec_per_sample(b.device.index, b._stream(), b.tree.data_ptr(), self.cap, ct.data_ptr(), k, beta,
                                  None if ut is None else ut.data_ptr(), seed, idx.data_ptr(), w.data_ptr())
        assert rc == 0, ctx
        self.check_draw(idx, w, k, u, counters[1], seed, beta, ctx)

    def zero_draws(self, ctx):
        self.buf._header()[X.HDR_DRAWS:X.HDR_DRAWS + 2].zero_()
        self.model.zero_draws()
        self.same(ctx)


@pytest.mark.parametrize("cap", X.CAPACITIES)
def test_scripted_sequence_is_the_model_bit_for_bit(cap):
    d = Device(cap)
    for n, op in enumerate(X.script(SEED, cap)):
        ctx = f"capacity {cap} op {n} {op['op']}"
        if op["op"] == "push":
            d.push(op["before"], op["after"], op["max_count"], ctx + f" {op['before'][:3]} -> {op['after'][:3]} max {op['max_count']}")
        elif op["op"] == "update":
            d.update(op["idx"], op["td"], op["alpha"], op["eps"], ctx + f" n {len(op['idx'])} alpha {op['alpha']}")
        elif op["op"] == "draw":
            d.draw(op["k"], op["u"], op["counters"], op["seed"], op["beta"], ctx + f" k {op['k']} u {'given' if op['u'] is not None else 'NULL'}")
        else:
            d.zero_draws(ctx)


def test_one_leaf_moved_by_a_thousandth_moves_all_four_ancestors():
    leaves, slot = X.single_leaf_case()
    d = Device(len(leaves))
    d.update(np.arange(len(leaves)), leaves, 1.0, 1e-30, "leaves near 1")
    m = d.model
    assert m.L == 4
    stale = [m.levels[l][slot >> (6 * l)] for l in range(m.L + 1)]
    d.update(np.array([slot]), np.array([stale[0] + np.float32(1e-3)], np.float32), 1.0, 1e-30, "one leaf")
    raw = d.raw()
    moved = 0
    for l in range(1, m.L + 1):
        node = slot >> (6 * l)
        got = raw[m.off[l] + node:m.off[l] + node + 1].view(np.float32)[0]
        assert got == m.levels[l][node], (l, got, m.levels[l][node])
        moved += got != stale[l]
        # what the 64-eps check of _per_reference.check_invariant makes of a node left stale: from level 2 up it passes
        kids = m.levels[l - 1][node * 64:node * 64 + 64].astype(np.float64).sum()
        assert (abs(float(stale[l]) - kids) <= 64 * R.EPS32 * kids) == (l >= 2), l
    assert moved >= 2 and stale[1] != m.levels[1][slot >> 6] and stale[2] != m.levels[2][slot >> 12]


@pytest.mark.parametrize("cap", [5000, 262145])
def test_the_class_on_a_ring_that_wraps_three_times(cap):
    import torch
    d = Device(cap, alpha=0.6, eps=1e-6, beta=0.4)
    buf, m = d.buf, d.model
    rng = np.random.default_rng(cap)
    chunk = cap * 3 // 8 + 1
    ring = [0, 0, 0, 0]
    zeros = lambda k: (torch.zeros(k, 1), torch.zeros(k, dtype=torch.int64), torch.zeros(k, dtype=torch.float64), torch.zeros(k, 1),
                       torch.zeros(k, dtype=torch.bool))
    buf.manual_seed(41)
    m.zero_draws()
    for rnd in range(9):
        ctx = f"capacity {cap} round {rnd}"
        buf.push_batch(*zeros(chunk))
        after = [(ring[0] + chunk) % cap, min(ring[1] + chunk, cap), ring[2] + chunk, 0]
        m.push(ring, after, min(chunk, cap))
        ring = after
        assert buf.counters.tolist() == ring, ctx
        d.same(ctx + " push_batch")
        k = 256
        out = buf.sample_prioritized(k)
        d.check_draw(out[5], out[6], k, None, ring[1], 41, 0.4, ctx + " sample_prioritized")
        idx = np.unique(out[5].cpu().numpy())
        td = (10.0 ** rng.uniform(-3, 2.5, len(idx))).astype(np.float32)
        td[int(rng.integers(0, len(idx)))] = np.float32(999.0)
        buf.update_priorities(torch.from_numpy(idx), torch.from_numpy(td))
        d.check_update(idx, td, 0.6, 1e-6, ctx + " update_priorities")
    assert ring[2] >= 3 * cap and buf.rejected_updates == 0
