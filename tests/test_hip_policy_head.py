"""The masked-categorical policy head on the GPU (gvec_policy_sample / _evaluate / _backward, MaskedCategoricalHead) against
the float64 numpy restatement of tests/_policy_reference.py.

Tolerances are measured, not chosen: on the same inputs torch's own float32 formulation (masked_fill -> log_softmax ->
entropy sum, and its autograd) is compared with the float64 reference, and the kernels may deviate at most 4 x as far
(floors 1e-6 forward, 1e-7 backward: about one float32 ulp of the values involved).  Every case prints both deviations."""
import ctypes as C
import functools

import numpy as np
import pytest

import _policy_reference as R

pytestmark = pytest.mark.gpu

CASES = [(rows, A, scale) for rows, A in R.SHAPES for scale in R.SCALES]


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


def hip_sample(logits, mask, seed, row_base=0, greedy=False):
    from generalsreinforcementlearning_amd._lib import PolicySampleArgs, check
    t = _torch()
    rows, A = logits.shape
    action = t.full((rows,), -7, dtype=t.int64, device=_dev())
    logp, ent = t.full((rows,), np.nan, device=_dev()), t.full((rows,), np.nan, device=_dev())
    a = PolicySampleArgs(rows=rows, num_actions=A, greedy=int(greedy), seed=seed, row_base=row_base, logits=_ptr(logits), mask=_ptr(mask),
                         action=_ptr(action), logp=_ptr(logp), entropy=_ptr(ent))
    check(_lib().gvec_policy_sample(0, _stream(), C.byref(a)), "gvec_policy_sample")
    return action, logp, ent


def hip_evaluate(logits, mask, action, bad=None):
    from generalsreinforcementlearning_amd._lib import PolicyEvaluateArgs, check
    t = _torch()
    rows, A = logits.shape
    logp, ent = t.full((rows,), np.nan, device=_dev()), t.full((rows,), np.nan, device=_dev())
    a = PolicyEvaluateArgs(rows=rows, num_actions=A, logits=_ptr(logits), mask=_ptr(mask), action=_ptr(action), logp=_ptr(logp),
                           entropy=_ptr(ent), bad_actions=_ptr(bad))
    check(_lib().gvec_policy_evaluate(0, _stream(), C.byref(a)), "gvec_policy_evaluate")
    return logp, ent


def hip_backward(logits, mask, action, gl, ge, out=None):
    from generalsreinforcementlearning_amd._lib import PolicyBackwardArgs, check
    t = _torch()
    rows, A = logits.shape
    if out is None:
        out = t.full((rows, A), np.nan, device=_dev())         # the kernel must overwrite every element
    a = PolicyBackwardArgs(rows=rows, num_actions=A, logits=_ptr(logits), mask=_ptr(mask), action=_ptr(action), grad_logp=_ptr(gl),
                           grad_entropy=_ptr(ge), grad_logits=_ptr(out))
    check(_lib().gvec_policy_backward(0, _stream(), C.byref(a)), "gvec_policy_backward")
    return out


def torch_forward(logits, mask):
    """The float32 formulation a user writes in torch: (logp [R, A], entropy [R]); NaN on dead rows."""
    t = _torch()
    lp = t.log_softmax(logits.masked_fill(mask == 0, float("-inf")), -1)
    return lp, -(lp.exp() * lp.masked_fill(lp == float("-inf"), 0.0)).sum(-1)


@functools.lru_cache(maxsize=None)
def case(rows, A, scale):
    """Inputs, the float64 reference and every device result of one case: computed once, shared by the tests below."""
    t = _torch()
    logits, mask, kind = R.case_inputs(rows, A, scale)
    rng = np.random.default_rng(rows + A)
    S = R.legal_set(logits, mask)
    live = S.any(1)
    action = np.array([rng.choice(np.flatnonzero(S[r])) if live[r] else 0 for r in range(rows)], np.int64)   # a legal action per live row
    w1, w2 = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    d = lambda x: t.as_tensor(x).to(_dev())
    c = dict(logits=logits, mask=mask, kind=kind, S=S, live=live, action=action, w1=w1, w2=w2,
             d_logits=d(logits), d_mask=d(mask), d_action=d(action), d_w1=d(w1), d_w2=d(w2))
    c["ref_logp_all"], _, c["ref_H"], c["dead"] = R.forward(logits, mask)
    c["ref_logp"], _, _ = R.evaluate(logits, mask, action)
    c["ref_grad"] = R.backward(logits, mask, action, w1, w2)
    # torch's float32 path and its autograd, on the same device
    tl = c["d_logits"].clone().requires_grad_(True)
    lp, ent = torch_forward(tl, c["d_mask"])
    c["torch_logp_all"], c["torch_H"] = lp.detach().cpu().numpy().astype(np.float64), ent.detach().cpu().numpy().astype(np.float64)
    lv = d(live)
    loss = (c["d_w1"] * lp.gather(1, c["d_action"][:, None]).squeeze(1) + c["d_w2"] * ent)[lv].sum()
    c["torch_grad"] = (t.autograd.grad(loss, tl)[0].cpu().numpy().astype(np.float64) if live.any() else np.zeros((rows, A)))
    return c


def _np(x):
    return x.cpu().numpy()


def forward_bounds(c):
    """(logp bound, entropy bound, torch's logp deviation, torch's entropy deviation) of a case: 4 x what torch's float32 path
    deviates from the float64 reference on every legal entry of the live rows' logp matrix and on their entropies."""
    live, S = c["live"], c["S"]
    with np.errstate(invalid="ignore"):             # -inf - -inf outside S: not looked at
        tdev_lp = np.abs(c["torch_logp_all"] - c["ref_logp_all"])[S].max() if live.any() else 0.0
    tdev_H = np.abs(c["torch_H"] - c["ref_H"])[live].max() if live.any() else 0.0
    return max(4 * tdev_lp, 1e-6), max(4 * tdev_H, 1e-6), tdev_lp, tdev_H


@pytest.mark.parametrize("rows,A,scale", CASES)
def test_evaluate_and_sample_match_the_reference(rows, A, scale):
    c = case(rows, A, scale)
    live, S = c["live"], c["S"]
    bound_lp, bound_H, tdev_lp, tdev_H = forward_bounds(c)
    logp, ent = map(_np, hip_evaluate(c["d_logits"], c["d_mask"], c["d_action"]))
    s_action, s_logp, s_ent = map(_np, hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED))
    s_ref_logp, _, s_bad = R.evaluate(c["logits"], c["mask"], s_action)
    kdev_lp = max(np.abs(logp - c["ref_logp"]).max(), np.abs(s_logp - s_ref_logp).max())
    kdev_H = max(np.abs(ent - c["ref_H"]).max(), np.abs(s_ent - c["ref_H"]).max())
    print(f"rows {rows} A {A} scale {scale}: logp dev kernel {kdev_lp:.3e} torch {tdev_lp:.3e}; entropy dev kernel {kdev_H:.3e} torch {tdev_H:.3e}")
    assert not s_bad.any()
    assert np.isfinite(logp).all() and np.isfinite(ent).all() and np.isfinite(s_logp).all() and np.isfinite(s_ent).all()
    assert kdev_lp <= bound_lp
    assert kdev_H <= bound_H
    # the exact cases
    dead = c["dead"]
    assert (logp[dead] == 0).all() and (ent[dead] == 0).all() and (s_logp[dead] == 0).all() and (s_ent[dead] == 0).all()
    assert (s_action[dead] == 0).all()
    single = S.sum(1) == 1
    assert (logp[single] == 0).all() and (ent[single] == 0).all() and (s_logp[single] == 0).all() and (s_ent[single] == 0).all()
    assert (s_action[single] == S[single].argmax(1)).all()
    const = (c["kind"] == R.ROW_KINDS.index("constant")) & live
    if const.any():
        assert np.abs(ent[const] - np.log(S[const].sum(1))).max() <= bound_H


@pytest.mark.parametrize("rows,A,scale", CASES)
def test_backward_matches_the_reference(rows, A, scale):
    c = case(rows, A, scale)
    live, S = c["live"], c["S"]
    tdev = np.abs(c["torch_grad"] - c["ref_grad"])[live].max() if live.any() else 0.0
    grad = _np(hip_backward(c["d_logits"], c["d_mask"], c["d_action"], c["d_w1"], c["d_w2"]))
    assert np.isfinite(grad).all(), "an element was left unwritten, or a NaN was computed"
    kdev = np.abs(grad - c["ref_grad"]).max()
    print(f"rows {rows} A {A} scale {scale}: grad dev kernel {kdev:.3e} torch {tdev:.3e}")
    assert kdev <= max(4 * tdev, 1e-7)
    assert (grad[~S] == 0).all()
    assert (grad[c["dead"]] == 0).all()
    assert (grad[S.sum(1) == 1] == 0).all()
    # either gradient may be NULL (= zeros)
    only_lp = _np(hip_backward(c["d_logits"], c["d_mask"], c["d_action"], c["d_w1"], None))
    only_H = _np(hip_backward(c["d_logits"], c["d_mask"], c["d_action"], None, c["d_w2"]))
    assert np.abs(only_lp - R.backward(c["logits"], c["mask"], c["action"], c["w1"], None)).max() <= max(4 * tdev, 1e-7)
    assert np.abs(only_H - R.backward(c["logits"], c["mask"], c["action"], None, c["w2"])).max() <= max(4 * tdev, 1e-7)
    assert (_np(hip_backward(c["d_logits"], c["d_mask"], c["d_action"], None, None)) == 0).all()


@pytest.mark.parametrize("rows,A,scale", CASES)
def test_sampling_matches_the_reference_draws(rows, A, scale):
    c = case(rows, A, scale)
    action, logp, _ = hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED)
    ref_action, key = R.sample(c["logits"], c["mask"], R.SAMPLING_SEED)
    a = _np(action)
    assert ((a >= 0) & (a < A)).all()
    assert (c["S"][np.arange(rows), a] | (c["dead"] & (a == 0))).all()
    differ = a != ref_action
    print(f"rows {rows} A {A} scale {scale}: {int(differ.sum())} rows off the float64 argmax")
    assert R.slack_ok(key, a)[differ].all()
    assert differ.sum() <= rows // 100
    ev_logp, _ = hip_evaluate(c["d_logits"], c["d_mask"], action)
    assert _torch().equal(logp, ev_logp)                       # bit for bit


def test_sampling_is_deterministic_and_keyed_by_row():
    t = _torch()
    rows, A, scale = 1000, 1125, 1.0
    c = case(rows, A, scale)
    first = hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED)
    again = hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED)
    assert all(t.equal(x, y) for x, y in zip(first, again))
    ev = [hip_evaluate(c["d_logits"], c["d_mask"], c["d_action"]) for _ in range(2)]
    assert t.equal(ev[0][0], ev[1][0]) and t.equal(ev[0][1], ev[1][1])
    bw = [hip_backward(c["d_logits"], c["d_mask"], c["d_action"], c["d_w1"], c["d_w2"]) for _ in range(2)]
    assert t.equal(bw[0], bw[1])
    half = rows // 2
    tail = hip_sample(c["d_logits"][half:], c["d_mask"][half:], R.SAMPLING_SEED, row_base=half)
    assert all(t.equal(x[half:], y) for x, y in zip(first, tail))
    other = hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED + 1)
    multi = c["S"].sum(1) >= 2
    changed = _np(first[0] != other[0])[multi]
    assert changed.mean() > 0.5, changed.mean()
    assert (_np(other[0]) == R.sample(c["logits"], c["mask"], R.SAMPLING_SEED + 1)[0]).mean() >= 0.99


def test_unaligned_base_pointers_change_nothing():
    """logits one float, the mask one byte, the gradient three floats off a 16-byte boundary: the same bits as aligned."""
    t = _torch()
    rows, A = 65, 1125
    c = case(rows, A, 1.0)
    buf = t.zeros(rows * A + 1, device=_dev())
    logits = buf[1:].view(rows, A)
    logits.copy_(c["d_logits"])
    mbuf = t.zeros(rows * A + 1, dtype=t.uint8, device=_dev())
    mask = mbuf[1:].view(rows, A)
    mask.copy_(c["d_mask"])
    assert logits.data_ptr() % 16 == 4 and mask.data_ptr() % 4 == 1 and c["d_logits"].data_ptr() % 16 == 0
    for x, y in zip(hip_sample(logits, mask, R.SAMPLING_SEED), hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED)):
        assert t.equal(x, y)
    for x, y in zip(hip_evaluate(logits, mask, c["d_action"]), hip_evaluate(c["d_logits"], c["d_mask"], c["d_action"])):
        assert t.equal(x, y)
    gbuf = t.full((rows * A + 3 + 4,), np.nan, device=_dev())
    out = gbuf[3:3 + rows * A].view(rows, A)
    hip_backward(logits, mask, c["d_action"], c["d_w1"], c["d_w2"], out=out)
    assert t.equal(out, hip_backward(c["d_logits"], c["d_mask"], c["d_action"], c["d_w1"], c["d_w2"]))
    assert t.isnan(gbuf[:3]).all() and t.isnan(gbuf[3 + rows * A:]).all()      # nothing outside the rows was written


def test_sampled_actions_follow_the_distribution():
    """65,536 rows share one 10-action row with 3 entries masked: no masked action is drawn and every legal action's count is
    within 5 binomial standard deviations of its expectation (fixed seed, deterministic kernel: this cannot flake)."""
    t = _torch()
    n = 65536
    row = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.7, -2.5, 1.6, 0.2], np.float32)
    m = np.array([1, 1, 0, 1, 1, 0, 1, 1, 0, 1], np.uint8)
    logits, mask = t.as_tensor(row).to(_dev()).repeat(n, 1).contiguous(), t.as_tensor(m).to(_dev()).repeat(n, 1).contiguous()
    action, _, _ = hip_sample(logits, mask, 20240607)
    counts = np.bincount(_np(action), minlength=10)
    _, p, _, _ = R.forward(row[None], m[None])
    p = p[0]
    assert counts[m == 0].sum() == 0
    sd = np.sqrt(n * p * (1 - p))
    z = np.abs(counts - n * p)[m != 0] / sd[m != 0]
    print("counts", counts, "z", np.round(z, 2))
    assert (z <= 5).all()


def test_greedy_takes_the_first_argmax():
    t = _torch()
    rows, A = 65, 320
    c = case(rows, A, 1.0)
    logits, mask = c["logits"].copy(), c["mask"].copy()
    # ties: the same maximum in two lanes (3 and 70), in one lane twice (5 and 69), and a masked greater value in front
    for r, (i, j) in zip((0, 9, 18), ((70, 3), (69, 5), (200, 131))):
        mask[r] = 1
        logits[r, [i, j]] = 50.0
        mask[r, 1] = 0
        logits[r, 1] = 99.0
    d_logits, d_mask = t.as_tensor(logits).to(_dev()), t.as_tensor(mask).to(_dev())
    action, logp, ent = hip_sample(d_logits, d_mask, 1, greedy=True)
    ref, _ = R.sample(logits, mask, 1, greedy=True)
    a = _np(action)
    assert (a == ref).all()
    assert a[0] == 3 and a[9] == 5 and a[18] == 131
    ev_logp, ev_ent = hip_evaluate(d_logits, d_mask, action)
    assert t.equal(logp, ev_logp) and t.equal(ent, ev_ent)
    assert t.equal(action, hip_sample(d_logits, d_mask, 2, greedy=True)[0])      # no draw is involved


def test_bad_actions_are_counted_and_carry_no_logp_gradient():
    t = _torch()
    rows, A = 65, 1125
    c = case(rows, A, 1.0)
    action = c["action"].copy()
    S, live = c["S"], c["live"]
    bad_rows = []
    for r in np.flatnonzero(live)[::3]:                        # a third of the live rows: out of range or illegal
        choice = [-1, A, 1 << 40, -(1 << 40)][len(bad_rows) % 4]
        illegal = np.flatnonzero(~S[r])
        action[r] = illegal[0] if (len(bad_rows) % 2 and len(illegal)) else choice
        bad_rows.append(r)
    action[~live] = [A + 5, 0, -3][0]                          # a dead row has no legal action: never counted
    d_action = t.as_tensor(action).to(_dev())
    bad = t.zeros(1, dtype=t.int64, device=_dev())
    logp, ent = hip_evaluate(c["d_logits"], c["d_mask"], d_action, bad)
    ref_logp, ref_H, ref_bad = R.evaluate(c["logits"], c["mask"], action)
    assert ref_bad.sum() == len(bad_rows) and int(bad.item()) == len(bad_rows)
    hip_evaluate(c["d_logits"], c["d_mask"], d_action, bad)
    assert int(bad.item()) == 2 * len(bad_rows)                # it accumulates
    hip_evaluate(c["d_logits"], c["d_mask"], d_action, None)   # NULL: not counted, not a fault
    assert (_np(logp)[bad_rows] == 0).all() and np.isfinite(_np(logp)).all()
    bound_lp, bound_H, _, _ = forward_bounds(c)
    assert np.abs(_np(logp) - ref_logp).max() <= bound_lp and np.abs(_np(ent) - ref_H).max() <= bound_H
    grad = _np(hip_backward(c["d_logits"], c["d_mask"], d_action, c["d_w1"], None))
    assert (grad[bad_rows] == 0).all() and (grad[~live] == 0).all()
    both = _np(hip_backward(c["d_logits"], c["d_mask"], d_action, c["d_w1"], c["d_w2"]))
    only_H = _np(hip_backward(c["d_logits"], c["d_mask"], d_action, None, c["d_w2"]))
    assert (both[bad_rows] == only_H[bad_rows]).all()


def test_autograd_through_the_head_is_the_backward_kernel():
    import generalsreinforcementlearning_amd as g
    t = _torch()
    B, L, A = 13, 5, 1125
    c = case(65, A, 1.0)
    head = g.MaskedCategoricalHead()
    logits = c["d_logits"].view(B, L, A).clone().requires_grad_(True)
    mask = c["d_mask"].view(B, L, A).view(t.bool)
    action, logp, ent = head.sample(logits, mask, seed=R.SAMPLING_SEED)
    assert action.shape == logp.shape == ent.shape == (B, L) and action.dtype == t.int64 and not logp.requires_grad
    direct = hip_sample(c["d_logits"], c["d_mask"], R.SAMPLING_SEED)
    assert t.equal(action.view(-1), direct[0]) and t.equal(logp.view(-1), direct[1]) and t.equal(ent.view(-1), direct[2])
    new_logp, new_ent = head.evaluate(logits, mask, action)
    assert new_logp.shape == new_ent.shape == (B, L) and t.equal(new_logp, logp) and t.equal(new_ent, ent)
    w1, w2 = c["d_w1"].view(B, L), c["d_w2"].view(B, L)
    grad, = t.autograd.grad((w1 * new_logp + w2 * new_ent).sum(), logits)
    assert grad.shape == (B, L, A)
    assert t.equal(grad.view(65, A), hip_backward(c["d_logits"], c["d_mask"], action.view(-1), c["d_w1"], c["d_w2"]))
    # only one of the two outputs in the loss, a non-contiguous float64 input, a greedy draw
    g1, = t.autograd.grad(head.evaluate(logits, mask, action)[1].sum(), logits)
    assert t.equal(g1.view(65, A), hip_backward(c["d_logits"], c["d_mask"], action.view(-1), None, t.ones(65, device=_dev())))
    wide = t.zeros(B, L, 2 * A, dtype=t.float64, device=_dev())
    wide[..., ::2] = logits.detach().double()
    lp64, _ = head.evaluate(wide[..., ::2], mask, action)
    assert t.equal(lp64, logp)
    assert t.equal(head.sample(logits, mask, seed=3, greedy=True)[0].view(-1), hip_sample(c["d_logits"], c["d_mask"], 3, greedy=True)[0])
    assert head.bad_actions == 0
    head.evaluate(logits, mask, t.full((B, L), A, dtype=t.int64, device=_dev()))
    assert head.bad_actions == int(c["live"].sum())
