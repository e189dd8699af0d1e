"""The policy-distillation loss without a GPU: the float64 restatement (tests/_distill_reference.py) against finite differences
of itself and against the definition's exact cases, the two C entry points' argument checks, and the ValueErrors of
MaskedCategoricalHead.distill, distill_loss and SelfPlayRolloutBuffer's policy-target arguments."""
import ctypes as C

import numpy as np
import pytest

import _distill_reference as D
import _policy_reference as R


def _inputs(rows=72, A=23, scale=1.0, seed=5):
    logits, mask, kind = R.make_rows(rows, A, scale, seed)
    target, tkind = D.make_targets(logits, mask, seed + 1)
    return logits, mask, kind, target, tkind


def test_make_targets_cycles_every_kind_over_every_row_kind():
    logits, mask, kind, target, tkind = _inputs()
    assert {(a, b) for a, b in zip(kind, tkind)} == {(a, b) for a in range(len(R.ROW_KINDS)) for b in range(len(D.TARGET_KINDS))}
    S = R.legal_set(logits, mask)
    k = lambda name: tkind == D.TARGET_KINDS.index(name)
    assert np.isnan(target[k("neg_nan")]).any() and (target[k("neg_nan")] < 0).any()
    assert (target[k("illegal_mass")][~S[k("illegal_mass")]] > 0).any()
    assert (target[k("tiny")] == np.float32(1e-30)).any()
    assert (target[k("zero")] == 0).all()
    live = S.any(1)
    assert np.allclose(D.tau_of(logits, mask, target)[k("half_mass") & live].sum(1), 0.5, atol=1e-6)
    assert ((target[k("one_hot")] != 0).sum(1) == 1).all()


def test_reference_gradient_is_the_finite_difference_of_its_own_outputs():
    """Central differences in float64, on rows whose logits are all finite (a -inf logit has no neighbourhood) and at a scale
    where the curvature term h^2 is far below the bound."""
    rng = np.random.default_rng(11)
    rows, A = 16, 9
    logits = rng.standard_normal((rows, A)).astype(np.float32)
    mask = (rng.random((rows, A)) < 0.6).astype(np.uint8)
    mask[0], mask[1], mask[2] = 1, 0, 0
    mask[2, 4] = 1                                            # rows 1 and 2: dead, a single legal action
    target, _ = D.make_targets(logits, mask, 12)
    w = rng.standard_normal((3, rows)).astype(np.float32)
    grad = D.backward(logits, mask, target, w[0], w[1], w[2])

    def loss(l):                                              # float64 throughout: R.forward widens whatever it is given
        lp, p, H, dead = _forward64(l, mask)
        tau = D.tau_of(logits, mask, target)
        pos = tau > 0
        ce = -(tau * np.where(pos, lp, 0.0)).sum(1)
        kl = (tau * (np.log(np.where(pos, tau, 1.0)) - np.where(pos, lp, 0.0))).sum(1)
        ce[dead], kl[dead] = 0.0, 0.0
        return (w[0] * ce + w[1] * kl + w[2] * H).sum()

    h = 1e-5
    fd = np.zeros((rows, A))
    base = logits.astype(np.float64)
    for r in range(rows):
        for i in range(A):
            up, dn = base.copy(), base.copy()
            up[r, i] += h
            dn[r, i] -= h
            fd[r, i] = (loss(up) - loss(dn)) / (2 * h)
    S = R.legal_set(logits, mask)
    assert np.abs(fd[~S]).max() == 0.0 and (grad[~S] == 0).all()
    assert np.abs(grad - fd).max() <= 1e-8, np.abs(grad - fd).max()
    ce, kl, H = D.forward(logits, mask, target)
    assert abs(loss(base) - (w[0] * ce + w[1] * kl + w[2] * H).sum()) <= 1e-12


def _forward64(l, mask):
    """_policy_reference.forward without its float32 rounding of the logits: what a finite difference needs."""
    S = (np.asarray(mask) != 0) & (l > -np.inf)
    dead = ~S.any(1)
    x = np.where(S, l, -np.inf)
    m = np.where(dead, 0.0, x.max(1, initial=-np.inf))
    e = np.where(S, np.exp(np.where(S, x - m[:, None], 0.0)), 0.0)
    Z = np.where(dead, 1.0, e.sum(1))
    logp = np.where(S, x - m[:, None] - np.log(Z)[:, None], -np.inf)
    p = np.where(S, np.exp(np.where(S, logp, 0.0)), 0.0)
    H = -(p * np.where(S, logp, 0.0)).sum(1)
    H[dead] = 0.0
    return logp, p, H, dead


def test_forward64_is_the_reference_forward_on_float32_inputs():
    logits, mask, _, _, _ = _inputs()
    a, b = R.forward(logits, mask), _forward64(logits.astype(np.float64), mask)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("scale", R.SCALES)
def test_kl_is_ce_minus_the_target_entropy_on_normalised_rows(scale):
    logits, mask, kind, target, tkind = _inputs(scale=scale)
    ce, kl, H = D.forward(logits, mask, target)
    tau = D.tau_of(logits, mask, target)
    _, _, _, dead = R.forward(logits, mask)
    normal = (np.abs(tau.sum(1) - 1.0) <= 1e-6) & ~dead
    assert normal.sum() >= 10
    assert np.abs(kl - (ce - D.target_entropy(logits, mask, target)))[normal].max() <= 1e-12
    assert (kl[normal] >= -1e-6).all()                          # a divergence, up to the float32 normalisation of the target


@pytest.mark.parametrize("scale", R.SCALES)
def test_the_exact_cases_of_the_definition(scale):
    logits, mask, kind, target, tkind = _inputs(scale=scale)
    rows, A = logits.shape
    ce, kl, H = D.forward(logits, mask, target)
    S = R.legal_set(logits, mask)
    logp, p, H0, dead = R.forward(logits, mask)
    assert np.array_equal(H, H0)
    w = np.random.default_rng(3).standard_normal((3, rows)).astype(np.float32)
    grad = D.backward(logits, mask, target, w[0], w[1], w[2])
    assert np.isfinite(ce).all() and np.isfinite(kl).all() and np.isfinite(grad).all()      # NaN targets, dead rows: never a NaN
    # dead rows: zeros
    assert dead.any() and (ce[dead] == 0).all() and (kl[dead] == 0).all() and (H[dead] == 0).all() and (grad[dead] == 0).all()
    assert (grad[~S] == 0).all()
    # a one-hot target at a legal action: ce = -logp of that action, exactly
    one = (tkind == D.TARGET_KINDS.index("one_hot")) & ~dead
    a = target[one].argmax(1)
    assert one.any() and np.array_equal(ce[one], -R.evaluate(logits[one], mask[one], a)[0])
    assert np.array_equal(kl[one], ce[one])                     # 1 * (log 1 - logp)
    # |S| = 1: ce = 0 and an exactly zero gradient, whatever the target's mass there
    single = S.sum(1) == 1
    assert single.any() and (ce[single] == 0).all() and (grad[single] == 0).all()
    # an all-zero target: ce = kl = 0, and the gradient is the entropy term alone
    zero = tkind == D.TARGET_KINDS.index("zero")
    assert (ce[zero] == 0).all() and (kl[zero] == 0).all()
    only_H = D.backward(logits, mask, target, None, None, w[2])
    assert np.array_equal(grad[zero], only_H[zero])
    assert (D.backward(logits, mask, target, w[0], w[1], None)[zero] == 0).all()
    # mass outside S, negative and NaN entries change nothing
    clean = np.where(S & (np.nan_to_num(target, nan=-1.0) > 0), target, np.float32(0))
    for x, y in zip(D.forward(logits, mask, target), D.forward(logits, mask, clean)):
        assert np.array_equal(x, y)
    # grad_ce and grad_kl act through their sum
    assert np.array_equal(D.backward(logits, mask, target, w[0], w[1], None), D.backward(logits, mask, target, w[1], w[0], None))
    assert np.array_equal(D.backward(logits, mask, target, w[0], None, w[2]), D.backward(logits, mask, target, None, w[0], w[2]))


def test_entry_points_check_their_arguments_before_any_device():
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import PolicyDistillArgs, PolicyDistillBackwardArgs
    L = g.load()
    p = 64                                                     # never dereferenced: the checks come first
    fwd = lambda **kw: PolicyDistillArgs(**{**dict(rows=4, num_actions=8, logits=p, mask=p, target=p, ce=p, kl=p, entropy=p), **kw})
    bwd = lambda **kw: PolicyDistillBackwardArgs(**{**dict(rows=4, num_actions=8, logits=p, mask=p, target=p, grad_ce=p, grad_kl=p,
                                                           grad_entropy=p, grad_logits=p), **kw})
    for fn, make, required in ((L.gvec_policy_distill, fwd, ("logits", "mask", "target", "ce", "kl", "entropy")),
                               (L.gvec_policy_distill_backward, bwd, ("logits", "mask", "target", "grad_logits"))):
        name = fn.__name__.encode()
        assert fn(0, None, None) == -1 and name in L.gvec_last_error()
        for bad in (dict(rows=-1), dict(rows=2 ** 31), dict(num_actions=0), dict(num_actions=-3)):
            assert fn(0, None, C.byref(make(**bad))) == -1, bad
            assert name in L.gvec_last_error() and b"rows" in L.gvec_last_error()
        for field in required:
            assert fn(0, None, C.byref(make(**{field: None}))) == -1, field
            assert name in L.gvec_last_error() and b"NULL" in L.gvec_last_error()
        assert fn(0, None, C.byref(make(rows=0))) == 0                                     # a no-op that needs no device
        assert fn(0, None, C.byref(make(rows=0, **{f: None for f in required}))) == 0      # ... and no pointers
        assert fn(0, None, C.byref(make(rows=0, num_actions=0))) == -1
    # the three upstream gradients may be NULL: not an argument error (without a device the call then fails on the device)
    import torch
    if not torch.cuda.is_available():
        assert L.gvec_policy_distill_backward(0, None, C.byref(bwd(grad_ce=None, grad_kl=None, grad_entropy=None))) not in (0, -1)


def test_distill_refuses_mismatched_inputs_before_any_library_call():
    import torch
    from generalsreinforcementlearning_amd import MaskedCategoricalHead, distill_loss
    logits, mask = torch.zeros(3, 2, 10), torch.ones(3, 2, 10, dtype=torch.bool)
    head = object.__new__(MaskedCategoricalHead)               # no device, no library: only the checks can run
    cases = [(logits, mask, torch.zeros(3, 2, 9)), (logits, mask, torch.zeros(6, 10)), (logits, mask, torch.zeros(3, 2, 10, dtype=torch.float64)),
             (logits, mask, torch.zeros(3, 2, 10, dtype=torch.float16)), (logits, mask[:, :1], torch.zeros(3, 2, 10)),
             (logits, mask, np.zeros((3, 2, 10), np.float32)), (torch.zeros(()), torch.ones((), dtype=torch.bool), torch.zeros(()))]
    for l, m, t in cases:
        with pytest.raises(ValueError):
            head.distill(l, m, t)
        with pytest.raises(ValueError):
            distill_loss(l, m, t)
    with pytest.raises(ValueError, match="weight"):
        distill_loss(logits, mask, torch.zeros(3, 2, 10), weight=torch.ones(3, 3))


def test_rollout_buffer_checks_its_policy_target_arguments():
    import torch
    from generalsreinforcementlearning_amd import SelfPlayRolloutBuffer

    class Env:                                                           # what the constructor reads before it allocates
        device_outputs, num_envs, num_learners, board_height, board_width = True, 4, 2, 5, 5
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="policy_target must be True or False"):
            SelfPlayRolloutBuffer(Env(), 4, policy_target=bad)

    def bare(has_target):                                                # step's checks read these and nothing else
        b = object.__new__(SelfPlayRolloutBuffer)
        b._t, b._has_target, b.num_envs, b.num_learners, b.num_streams, b.mask_bytes = torch, has_target, 4, 2, 8, 125
        return b
    z = torch.zeros(8)
    with pytest.raises(ValueError, match="needs the step's policy_target"):
        bare(True).step(z.long(), z, z)
    with pytest.raises(ValueError, match="needs the step's policy_target"):
        bare(True).step(z.long(), z, z, search_value=z)
    for target in (torch.zeros(4, 2, 124), torch.zeros(4, 2, 125, dtype=torch.float64), torch.zeros(4, 125), np.zeros((4, 2, 125), np.float32),
                   torch.zeros(2, 4, 5, 25)):
        with pytest.raises(ValueError, match="policy_target must be a float32 tensor"):
            bare(True).step(z.long(), z, z, policy_target=target)
    with pytest.raises(ValueError, match="search_value"):
        bare(True).step(z.long(), z, z, policy_target=torch.zeros(4, 2, 125), search_value=torch.zeros(7))
    with pytest.raises(ValueError, match="policy_target=False"):
        bare(False).step(z.long(), z, z, policy_target=torch.zeros(4, 2, 125))
    with pytest.raises(ValueError, match="policy_target=False"):
        bare(False).step(z.long(), z, z, search_value=z)
