"""A float64 numpy model of prioritized replay over a ring, written from the specification of the sum tree (radix 64, one
leaf per slot, stratified draws, importance weights normalised by the batch's largest) and not from the kernels."""
import numpy as np

EPS32 = 2.0 ** -24


def prefix(leaves):
    """F[0] = 0, F[i + 1] = F[i] + leaf[i] in float64 (exact to 2^-53 relative per term)."""
    F = np.zeros(len(leaves) + 1, np.float64)
    np.cumsum(np.asarray(leaves, np.float64), out=F[1:])
    return F


def targets(k, u, total):
    """Draw j aims at (j + u[j]) / k of the total."""
    return (np.arange(k, dtype=np.float64) + np.asarray(u, np.float64)) / k * total


def bracket(F, t):
    """The slot i with F[i] <= t < F[i + 1]."""
    return np.searchsorted(F, t, side="right") - 1


def leaf_value(td, alpha, eps):
    return (np.abs(np.asarray(td, np.float64)) + eps) ** alpha


def weights(leaves, idx, size, beta):
    """(size * P(i)) ** -beta over the batch's largest, P(i) = leaf_i / total."""
    leaves = np.asarray(leaves, np.float64)
    w = (size * leaves[idx] / leaves.sum()) ** -beta
    return w / w.max()


def slack(levels, total):
    """2 L 64 eps total: one L 64 eps for the tree's float32 sums, one for the descent's subtractions."""
    return 2.0 * levels * 64 * EPS32 * total


def read_tree(buf):
    """The levels of a PrioritizedDeviceReplayBuffer's tree as float64 host arrays (level 0 = leaves, unpadded), and the maximum."""
    import torch
    raw = buf.tree.cpu()
    n, out = buf.capacity, []
    for l, off in enumerate(buf.tree_offsets):
        out.append(raw[off:off + n].numpy().astype(np.float64))
        pad = raw[off + n:off + (n + 63) // 64 * 64]
        assert not pad.any(), f"level {l}: padding is not zero"
        n = (n + 63) // 64
    top = float(raw[:1].view(torch.int32).view(torch.float32)[0])
    return out, top


def check_invariant(buf, ctx=""):
    """Every node equals the float64 sum of its 64 children within 64 eps relative; returns (leaves, maximum)."""
    lv, top = read_tree(buf)
    for l in range(1, len(lv)):
        kids = lv[l - 1]
        padded = np.zeros((len(kids) + 63) // 64 * 64)
        padded[:len(kids)] = kids
        want = padded.reshape(-1, 64).sum(1)
        assert len(want) == len(lv[l])
        bad = np.abs(lv[l] - want) > 64 * EPS32 * want
        assert not bad.any(), f"{ctx}: level {l}: {int(bad.sum())} nodes off, first {np.flatnonzero(bad)[:5]}"
    assert len(lv[-1]) == 1
    return lv[0], top
