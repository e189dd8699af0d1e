"""CPU-side checks of the policy head: the numpy reference is consistent with itself, the sampling test's inputs leave
its slack route rare, and the three entry points refuse bad arguments before anything touches a device."""
import ctypes as C

import numpy as np

import _policy_reference as R


def test_reference_gradient_matches_finite_differences():
    """The analytic gradient of w1 * logp[a] + w2 * H against central differences of the reference's own float64 forward."""
    rng = np.random.default_rng(7)
    rows, A = 6, 7
    logits = rng.standard_normal((rows, A)).astype(np.float32)
    mask = np.ones((rows, A), np.uint8)
    for r in range(rows):
        mask[r, rng.choice(A, 3, replace=False)] = 0
    action = np.array([np.flatnonzero(mask[r])[r % 4] for r in range(rows)])
    w1, w2 = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    grad = R.backward(logits, mask, action, w1, w2)

    def f(l):                                     # float64 all the way: the forward's float32 cast is bypassed
        S = mask != 0
        x = np.where(S, l, -np.inf)
        m = x.max(1, keepdims=True)
        logp = x - m - np.log(np.exp(x - m).sum(1, keepdims=True))
        p = np.where(S, np.exp(logp), 0.0)
        H = -(p * np.where(S, logp, 0.0)).sum(1)
        return w1 * logp[np.arange(rows), action] + w2 * H

    l64, eps = logits.astype(np.float64), 1e-6
    for i in range(A):
        d = np.zeros((rows, A))
        d[:, i] = eps
        fd = (f(l64 + d) - f(l64 - d)) / (2 * eps)
        if (mask[:, i] == 0).any():
            assert (grad[mask[:, i] == 0, i] == 0).all()
        live = mask[:, i] != 0
        assert np.abs(fd[live] - grad[live, i]).max() < 1e-8, (i, fd, grad[:, i])


def test_sampling_inputs_keep_the_slack_route_under_its_cap():
    """tests/test_hip_policy_head.py lets a row pass when the kernel's pick differs from the float64 argmax but its float64
    key is within 2^-20 * max(1, |best|) of the best - for at most 1 % of a case's rows.  Here the draw and the add are redone
    in float32 on exactly those inputs and that seed: float32's disagreement with float64 stays within the cap on every
    case, so an honest float32 kernel does not need more."""
    worst = 0.0
    for rows, A in R.SHAPES:
        for scale in R.SCALES:
            logits, mask, _ = R.case_inputs(rows, A, scale)
            a64, key = R.sample(logits, mask, R.SAMPLING_SEED)
            a32, _ = R.sample(logits, mask, R.SAMPLING_SEED, f32=True)
            differ = int((a64 != a32).sum())
            worst = max(worst, differ / rows)
            assert differ <= rows // 100, (rows, A, scale, differ)
            legal = R.legal_set(logits, mask)
            assert (legal[np.arange(rows), a64] | ~legal.any(1)).all()
    print(f"float32 vs float64 sampling: worst share of differing rows {worst:.4f}")


def test_draws_are_keyed_by_seed_row_and_element_alone():
    k = R.draws24(R.SAMPLING_SEED, np.arange(8, dtype=np.int64), 11)
    assert (R.draws24(R.SAMPLING_SEED, np.arange(4, 8, dtype=np.int64), 11) == k[4:]).all()
    assert (R.draws24(R.SAMPLING_SEED, np.arange(8, dtype=np.int64), 5) == k[:, :5]).all()
    assert (R.draws24(R.SAMPLING_SEED + 1, np.arange(8, dtype=np.int64), 11) != k).mean() > 0.9
    assert k.min() >= 0 and k.max() < 1 << 24


def test_policy_entry_points_validate_their_arguments_without_a_gpu():
    """-1 with a message for bad arguments, 0 for rows == 0: both before anything touches a device."""
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import PolicyBackwardArgs, PolicyEvaluateArgs, PolicySampleArgs
    L = g.load()
    p = 16                                        # never dereferenced
    full = {
        "gvec_policy_sample": (PolicySampleArgs, dict(logits=p, mask=p, action=p, logp=p, entropy=p), ()),
        "gvec_policy_evaluate": (PolicyEvaluateArgs, dict(logits=p, mask=p, action=p, logp=p, entropy=p), ("bad_actions",)),
        "gvec_policy_backward": (PolicyBackwardArgs, dict(logits=p, mask=p, action=p, grad_logits=p), ("grad_logp", "grad_entropy")),
    }
    for name, (cls, ptrs, optional) in full.items():
        fn = getattr(L, name)
        assert fn(0, None, None) == -1 and name.encode() in L.gvec_last_error()
        for rows, A in ((4, 0), (4, -3), (-1, 5), (1 << 31, 5)):
            assert fn(0, None, C.byref(cls(rows=rows, num_actions=A, **ptrs))) == -1, (name, rows, A)
            assert name.encode() in L.gvec_last_error()
        for missing in ptrs:
            a = cls(rows=4, num_actions=5, **{k: v for k, v in ptrs.items() if k != missing})
            assert fn(0, None, C.byref(a)) == -1 and b"NULL" in L.gvec_last_error(), (name, missing)
        assert fn(0, None, C.byref(cls(rows=0, num_actions=5, **ptrs))) == 0          # nothing to do: no device needed
        assert fn(0, None, C.byref(cls(rows=0, num_actions=0, **ptrs))) == -1         # the shape is checked first
        for o in optional:
            assert getattr(cls(rows=0, num_actions=5, **ptrs), o) is None
    assert L.gvec_abi_version() == 2


def test_head_needs_a_gpu():
    import pytest
    import torch
    import generalsreinforcementlearning_amd as g
    if torch.cuda.is_available():
        g.MaskedCategoricalHead()
        return
    with pytest.raises(g.GvecError) as ei:
        g.MaskedCategoricalHead()
    assert ei.value.code == -2
