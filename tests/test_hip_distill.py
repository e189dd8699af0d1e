"""The policy-distillation kernels on the GPU (gvec_policy_distill / gvec_policy_distill_backward, MaskedCategoricalHead.distill,
distill_loss) against the float64 numpy restatement of tests/_distill_reference.py.

Tolerances are measured as tests/test_hip_policy_head.py measures them: on the same inputs the float32 formulation a user writes
in torch (masked_fill -> log_softmax -> (target * logp).sum -> xlogy, and its autograd) is compared with the float64 reference,
and the kernels may deviate at most 4 x as far (floors 1e-6 forward, 1e-7 backward).  Rows where torch yields NaN (dead rows)
are excluded from torch's side only.  Every case prints both deviations."""
import ctypes as C
import functools

import numpy as np
import pytest

import _distill_reference as D
import _policy_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(65, A) for A in (1, 5, 63, 64, 65, 320, 1125, 5120)] + [(1, 1125), (1000, 1125), (3, 5121)]
CASES = [(rows, A, scale) for rows, A in SHAPES for scale in R.SCALES]


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _lib():
    import generalsreinforcementlearning_amd as g
    return g.load()


def _stream():
    return _torch().cuda.current_stream(_dev()).cuda_stream


def _ptr(x):
    return None if x is None else x.data_ptr()


def _np(x):
    return x.cpu().numpy()


def hip_distill(logits, mask, target):
    from generalsreinforcementlearning_amd._lib import PolicyDistillArgs, check
    t = _torch()
    rows, A = logits.shape
    ce, kl, ent = (t.full((rows,), np.nan, device=_dev()) for _ in range(3))
    a = PolicyDistillArgs(rows=rows, num_actions=A, logits=_ptr(logits), mask=_ptr(mask), target=_ptr(target), ce=_ptr(ce), kl=_ptr(kl),
                          entropy=_ptr(ent))
    check(_lib().gvec_policy_distill(0, _stream(), C.byref(a)), "gvec_policy_distill")
    return ce, kl, ent


def hip_distill_backward(logits, mask, target, gc, gk, ge, out=None):
    from generalsreinforcementlearning_amd._lib import PolicyDistillBackwardArgs, check
    t = _torch()
    rows, A = logits.shape
    if out is None:
        out = t.full((rows, A), np.nan, device=_dev())         # the kernel must overwrite every element
    a = PolicyDistillBackwardArgs(rows=rows, num_actions=A, logits=_ptr(logits), mask=_ptr(mask), target=_ptr(target), grad_ce=_ptr(gc),
                                  grad_kl=_ptr(gk), grad_entropy=_ptr(ge), grad_logits=_ptr(out))
    check(_lib().gvec_policy_distill_backward(0, _stream(), C.byref(a)), "gvec_policy_distill_backward")
    return out


def hip_evaluate(logits, mask, action):
    from generalsreinforcementlearning_amd._lib import PolicyEvaluateArgs, check
    t = _torch()
    rows, A = logits.shape
    logp, ent = t.full((rows,), np.nan, device=_dev()), t.full((rows,), np.nan, device=_dev())
    a = PolicyEvaluateArgs(rows=rows, num_actions=A, logits=_ptr(logits), mask=_ptr(mask), action=_ptr(action), logp=_ptr(logp),
                           entropy=_ptr(ent), bad_actions=None)
    check(_lib().gvec_policy_evaluate(0, _stream(), C.byref(a)), "gvec_policy_evaluate")
    return logp, ent


def torch_distill(logits, mask, target):
    """The float32 formulation a user writes in torch: (ce, kl, entropy) [R]; NaN on dead rows.  The user cleans the target the
    way the definition does (legal and > 0), or the NaN entries of the test's targets would be all there is to see."""
    t = _torch()
    lp = t.log_softmax(logits.masked_fill(mask == 0, float("-inf")), -1)
    tau = t.where((lp > float("-inf")) & (target > 0), target, t.zeros_like(target))      # S: legal and a logit above -inf
    lp0 = lp.masked_fill(lp == float("-inf"), 0.0)
    ce = -(tau * lp0).sum(-1)
    kl = t.xlogy(tau, tau).sum(-1) + ce
    ent = -(lp.exp() * lp0).sum(-1)
    return ce, kl, ent


@functools.lru_cache(maxsize=None)
def case(rows, A, scale):
    """Inputs, the float64 reference and torch's float32 results of one case: computed once, shared by the tests below."""
    t = _torch()
    logits, mask, kind = R.case_inputs(rows, A, scale)
    target, tkind = D.make_targets(logits, mask, seed=rows * 31 + A)
    rng = np.random.default_rng(rows + A + 1)
    S = R.legal_set(logits, mask)
    live = S.any(1)
    w = [rng.standard_normal(rows).astype(np.float32) for _ in range(3)]
    d = lambda x: t.as_tensor(x).to(_dev())
    c = dict(logits=logits, mask=mask, target=target, kind=kind, tkind=tkind, S=S, live=live, dead=~live, w=w,
             d_logits=d(logits), d_mask=d(mask), d_target=d(target), d_w=[d(x) for x in w])
    c["ref"] = D.forward(logits, mask, target)
    c["ref_grad"] = D.backward(logits, mask, target, *w)
    tl = c["d_logits"].clone().requires_grad_(True)
    out = torch_distill(tl, c["d_mask"], c["d_target"])
    c["torch"] = [x.detach().cpu().numpy().astype(np.float64) for x in out]
    lv = d(live)
    loss = sum((wi * x)[lv].sum() for wi, x in zip(c["d_w"], out))
    c["torch_grad"] = t.autograd.grad(loss, tl)[0].cpu().numpy().astype(np.float64) if live.any() else np.zeros((rows, A))
    return c


def _dev_max(x, ref, rows):
    return float(np.abs(x - ref)[rows].max()) if rows.any() else 0.0


@pytest.mark.parametrize("rows,A,scale", CASES)
def test_forward_matches_the_reference(rows, A, scale):
    c = case(rows, A, scale)
    live, dead, S = c["live"], c["dead"], c["S"]
    t = _torch()
    out = [_np(x) for x in hip_distill(c["d_logits"], c["d_mask"], c["d_target"])]
    assert all(np.isfinite(x).all() for x in out), "an output was left unwritten, or a NaN was computed"
    for name, k, ref, tor in zip(("ce", "kl", "entropy"), out, c["ref"], c["torch"]):
        tdev = _dev_max(tor, ref, live & np.isfinite(tor))
        kdev = _dev_max(k, ref, np.ones(rows, bool))
        print(f"rows {rows} A {A} scale {scale}: {name} dev kernel {kdev:.3e} torch {tdev:.3e}")
        assert kdev <= max(4 * tdev, 1e-6), name
    ce, kl, ent = out
    # the exact cases
    assert (ce[dead] == 0).all() and (kl[dead] == 0).all() and (ent[dead] == 0).all()
    single = S.sum(1) == 1
    assert (ce[single] == 0).all() and (ent[single] == 0).all()
    zero = c["tkind"] == D.TARGET_KINDS.index("zero")
    assert (ce[zero] == 0).all() and (kl[zero] == 0).all()
    # a one-hot target at a legal action: -logp of gvec_policy_evaluate for that action, to the bit
    one = (c["tkind"] == D.TARGET_KINDS.index("one_hot")) & live
    action = t.as_tensor(np.where(one, np.nan_to_num(c["target"]).argmax(1), 0).astype(np.int64)).to(_dev())
    logp, ev_ent = (_np(x) for x in hip_evaluate(c["d_logits"], c["d_mask"], action))
    assert ((-logp[one]).view(np.int32) == ce[one].view(np.int32)).all()
    assert (kl[one] == ce[one]).all()                                  # 1 * (log 1 - logp)
    assert (ev_ent.view(np.int32) == ent.view(np.int32)).all()         # the entropy is gvec_policy_evaluate's


@pytest.mark.parametrize("rows,A,scale", CASES)
def test_backward_matches_the_reference(rows, A, scale):
    c = case(rows, A, scale)
    live, dead, S = c["live"], c["dead"], c["S"]
    tdev = np.abs(c["torch_grad"] - c["ref_grad"])[live].max() if live.any() else 0.0
    bound = max(4 * tdev, 1e-7)
    args = (c["d_logits"], c["d_mask"], c["d_target"])
    grad = _np(hip_distill_backward(*args, *c["d_w"]))
    assert np.isfinite(grad).all(), "an element was left unwritten, or a NaN was computed"
    kdev = np.abs(grad - c["ref_grad"]).max()
    print(f"rows {rows} A {A} scale {scale}: grad dev kernel {kdev:.3e} torch {tdev:.3e}")
    assert kdev <= bound
    assert (grad[~S] == 0).all()
    assert (grad[dead] == 0).all()
    assert (grad[S.sum(1) == 1] == 0).all()                    # one legal action: Tsum = tau, p = 1, H = 0
    # each of the three gradients NULL (= zeros) in turn, and all three
    for skip in range(3):
        dw = [None if i == skip else x for i, x in enumerate(c["d_w"])]
        w = [None if i == skip else x for i, x in enumerate(c["w"])]
        got = _np(hip_distill_backward(*args, *dw))
        assert np.isfinite(got).all()
        assert np.abs(got - D.backward(c["logits"], c["mask"], c["target"], *w)).max() <= bound, skip
    assert (_np(hip_distill_backward(*args, None, None, None)) == 0).all()


def test_results_are_deterministic():
    t = _torch()
    c = case(1000, 1125, 1.0)
    args = (c["d_logits"], c["d_mask"], c["d_target"])
    a, b = hip_distill(*args), hip_distill(*args)
    assert all(t.equal(x, y) for x, y in zip(a, b))
    assert t.equal(hip_distill_backward(*args, *c["d_w"]), hip_distill_backward(*args, *c["d_w"]))


@pytest.mark.parametrize("A", (1125, 64, 5121))
def test_unaligned_base_pointers_change_nothing(A):
    """logits, mask, target and gradient 1 to 3 elements off a 16-byte boundary, each by another amount: the same bits."""
    t = _torch()
    rows = 65 if A != 5121 else 3
    c = case(rows, A, 1.0)

    def shifted(x, off, dtype, fill=0):
        buf = t.full((rows * A + off + 4,), fill, dtype=dtype, device=_dev())
        v = buf[off:off + rows * A].view(rows, A)
        if x is not None:
            v.copy_(x)
        return buf, v

    base = hip_distill(c["d_logits"], c["d_mask"], c["d_target"])
    base_grad = hip_distill_backward(c["d_logits"], c["d_mask"], c["d_target"], *c["d_w"])
    for lo, mo, to, go in ((1, 1, 2, 3), (2, 3, 1, 1), (3, 2, 3, 2), (0, 1, 3, 0), (1, 0, 0, 2)):
        _, logits = shifted(c["d_logits"], lo, t.float32)
        _, mask = shifted(c["d_mask"], mo, t.uint8)
        _, target = shifted(c["d_target"], to, t.float32)
        assert logits.data_ptr() % 16 == 4 * lo and target.data_ptr() % 16 == 4 * to and mask.data_ptr() % 4 == mo
        for x, y in zip(hip_distill(logits, mask, target), base):
            assert t.equal(x, y), (lo, mo, to)
        gbuf, out = shifted(None, go, t.float32, fill=np.nan)
        hip_distill_backward(logits, mask, target, *c["d_w"], out=out)
        assert t.equal(out, base_grad), (lo, mo, to, go)
        assert t.isnan(gbuf[:go]).all() and t.isnan(gbuf[go + rows * A:]).all()      # nothing outside the rows was written


def test_autograd_through_distill_is_the_backward_kernel():
    import generalsreinforcementlearning_amd as g
    t = _torch()
    B, L, A = 13, 5, 1125
    c = case(65, A, 1.0)
    head = g.MaskedCategoricalHead()
    logits = c["d_logits"].view(B, L, A).clone().requires_grad_(True)
    mask = c["d_mask"].view(B, L, A).view(t.bool)
    target = c["d_target"].view(B, L, A)
    ce, kl, ent = head.distill(logits, mask, target)
    assert ce.shape == kl.shape == ent.shape == (B, L) and ce.requires_grad
    direct = hip_distill(c["d_logits"], c["d_mask"], c["d_target"])
    assert all(t.equal(x.reshape(-1), y) for x, y in zip((ce, kl, ent), direct))
    w = [x.view(B, L) for x in c["d_w"]]
    grad, = t.autograd.grad((w[0] * ce + w[1] * kl + w[2] * ent).sum(), logits)
    assert grad.shape == (B, L, A)
    assert t.equal(grad.view(65, A), hip_distill_backward(c["d_logits"], c["d_mask"], c["d_target"], *c["d_w"]))
    # one output alone in the loss; the target takes no gradient; a non-contiguous float64 logits input
    g1, = t.autograd.grad(head.distill(logits, mask, target)[0].sum(), logits)
    ones, zeros = t.ones(65, device=_dev()), t.zeros(65, device=_dev())
    assert t.equal(g1.view(65, A), hip_distill_backward(c["d_logits"], c["d_mask"], c["d_target"], ones, zeros, zeros))
    tg = target.clone().requires_grad_(True)
    out = head.distill(logits, mask, tg)[0].sum()
    assert t.autograd.grad(out, tg, allow_unused=True)[0] is None
    wide = t.zeros(B, L, 2 * A, dtype=t.float64, device=_dev())
    wide[..., ::2] = logits.detach().double()
    assert t.equal(head.distill(wide[..., ::2], mask, target)[0], ce)
    # rows == 0: zeros that carry a graph
    empty = t.zeros(0, 7, A, device=_dev(), requires_grad=True)
    e = head.distill(empty, t.zeros(0, 7, A, dtype=t.bool, device=_dev()), t.zeros(0, 7, A, device=_dev()))
    assert all(x.shape == (0, 7) and x.requires_grad for x in e)
    assert t.autograd.grad(e[0].sum() + e[1].sum(), empty)[0].shape == (0, 7, A)
    with pytest.raises(ValueError):
        head.distill(logits, mask, target.double())


def test_distill_loss_is_the_weighted_mean_of_ce():
    import generalsreinforcementlearning_amd as g
    t = _torch()
    c = case(65, 1125, 1.0)
    ce = hip_distill(c["d_logits"], c["d_mask"], c["d_target"])[0]
    logits = c["d_logits"].clone().requires_grad_(True)
    mask, target = c["d_mask"].view(t.bool), c["d_target"]
    w = (t.arange(65, device=_dev()) % 3 != 0).float()
    loss = g.distill_loss(logits, mask, target, w)
    assert loss.shape == () and t.equal(loss, (w * ce).sum() / w.sum().clamp(min=1.0))
    assert t.equal(g.distill_loss(logits, mask, target), ce.sum() / 65)
    small = w * 1e-3                                           # a weight sum below 1: the denominator is clamped at 1
    assert t.equal(g.distill_loss(logits, mask, target, small), (small * ce).sum())
    assert g.distill_loss(logits, mask, target, t.zeros(65, device=_dev())).detach().item() == 0.0
    grad, = t.autograd.grad(loss, logits)
    gc = w / w.sum().clamp(min=1.0)
    assert t.equal(grad, hip_distill_backward(c["d_logits"], c["d_mask"], c["d_target"], gc, t.zeros_like(gc), t.zeros_like(gc)))
