"""The policy-distillation loss (gvec_policy_distill / _backward) restated in numpy, float64 from the float32 inputs, written
from include/generals_vec.h "policy distillation" and DESIGN.md section 4.23 on top of _policy_reference.forward - not from
the kernels.

Also the shared targets of the CPU and GPU tests: `make_targets` cycles every kind of target row over whatever rows
_policy_reference.make_rows dealt."""
import numpy as np

import _policy_reference as R


def tau_of(logits, mask, target):
    """tau [R, A] float64: the target where the action is in S and the entry is > 0, otherwise 0 (NaN and negatives dropped)."""
    t = np.asarray(target, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = R.legal_set(np.asarray(logits, np.float32), mask) & (t > 0)
    return np.where(keep, t, 0.0)


def forward(logits, mask, target):
    """(ce [R], kl [R], H [R]); a dead row gives zeros."""
    logp, _, H, dead = R.forward(logits, mask)
    tau = tau_of(logits, mask, target)
    pos = tau > 0
    lp = np.where(pos, logp, 0.0)
    ce = -(tau * lp).sum(1)
    kl = (tau * (np.log(np.where(pos, tau, 1.0)) - lp)).sum(1)
    ce[dead] = 0.0
    kl[dead] = 0.0
    return ce, kl, H


def target_entropy(logits, mask, target):
    tau = tau_of(logits, mask, target)
    return -(tau * np.log(np.where(tau > 0, tau, 1.0))).sum(1)


def backward(logits, mask, target, grad_ce=None, grad_kl=None, grad_entropy=None):
    """grad_logits [R, A] float64: i in S: g * (Tsum * p_i - tau_i) - (ge * p_i) * (logp_i + H), g = grad_ce + grad_kl; else 0."""
    logp, p, H, dead = R.forward(logits, mask)
    S = R.legal_set(np.asarray(logits, np.float32), mask)
    rows = logp.shape[0]
    f = lambda g: np.zeros(rows) if g is None else np.asarray(g, np.float32).astype(np.float64)
    g, ge = f(grad_ce) + f(grad_kl), f(grad_entropy)
    tau = tau_of(logits, mask, target)
    out = g[:, None] * (tau.sum(1)[:, None] * p - tau) - (ge[:, None] * p) * (np.where(S, logp, 0.0) + H[:, None])
    return np.where(S & ~dead[:, None], out, 0.0)


TARGET_KINDS = ["dense", "one_hot", "sparse16", "zero", "half_mass", "illegal_mass", "neg_nan", "tiny"]


def make_targets(logits, mask, seed):
    """(target float32 [R, A], kind [R]).  Row r is of kind TARGET_KINDS[(r // 9 + r % 9) % 8]: _policy_reference.make_rows
    cycles its 9 row kinds with r % 9, so over 72 rows every row kind meets every target kind.  A dead row gets its kind's pattern on
    arbitrary entries: all of it is dropped."""
    rng = np.random.default_rng(seed)
    l = np.asarray(logits, np.float32)
    rows, A = l.shape
    S = R.legal_set(l, mask)
    target = np.zeros((rows, A), np.float32)
    kind = np.array([(r // 9 + r % 9) % len(TARGET_KINDS) for r in range(rows)])

    def dense(r, idx):
        z = np.where(np.isfinite(l[r, idx]), l[r, idx], 0.0).astype(np.float64) + rng.standard_normal(len(idx))
        e = np.exp(z - z.max())
        return (e / e.sum()).astype(np.float32)

    for r in range(rows):
        legal = np.flatnonzero(S[r])
        idx = legal if len(legal) else np.arange(A)
        k = TARGET_KINDS[kind[r]]
        if k == "dense":                                      # what gvec_search_improved_policy writes: softmax over S of logits + noise
            target[r, idx] = dense(r, idx)
        elif k == "one_hot":
            target[r, rng.choice(idx)] = 1.0
        elif k == "sparse16":
            pick = rng.choice(idx, min(16, len(idx)), replace=False)
            w = rng.random(len(pick)) + 0.05
            target[r, pick] = (w / w.sum()).astype(np.float32)
        elif k == "zero":
            pass
        elif k == "half_mass":                                # unnormalised: sums to 0.5
            target[r, idx] = dense(r, idx) * np.float32(0.5)
        elif k == "illegal_mass":                             # every entry positive: whatever lies outside S is dropped
            target[r] = (rng.random(A) + 0.01).astype(np.float32) / np.float32(A)
        elif k == "neg_nan":
            target[r, idx] = dense(r, idx)
            bad = rng.choice(A, max(1, A // 4), replace=False)
            target[r, bad[::2]] = -np.abs(rng.standard_normal(len(bad[::2]))).astype(np.float32) - np.float32(0.01)
            target[r, bad[1::2]] = np.nan
        elif k == "tiny":
            target[r, idx] = dense(r, idx)
            target[r, rng.choice(idx)] = np.float32(1e-30)
    return target, kind
