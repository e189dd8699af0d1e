"""gvec_search_halve and gvec_search_improved_policy on the GPU against the numpy restatement (tests/_halving_reference.py) on
synthetic buffers - halve bit for bit, the policy target within a bound measured on each case's inputs - and HalvingSearch
end to end on small engines: equal to PlayoutSearch.evaluate driven round by round with the restatement choosing the
survivors, repeatable, read-only on its roots, and right in a position whose answer is known."""
import ctypes as C

import numpy as np
import pytest

import _halving_reference as HR
import _search_reference as SR

pytestmark = pytest.mark.gpu

WEIGHTS = dict(win=2.0, loss=-1.5, land=0.25, army=1.0)          # not the defaults: every weight is read
C_VISIT, C_SCALE = 50.0, 1.0
SENTINEL = -77


def _cuda(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- halve: bit for bit -----------------------------------------------------------------------------------------------------
def _halve_case(n, k, R, m, identity, seed):
    """Rows of every kind in one batch.  Per row r: r % 5 == 1 all playouts valid, == 2 all invalid, otherwise a mix per
    column - invalid columns, GVEC_SEARCH_NONE padding, pairs of columns with equal keys (the same terms, prior and history),
    won and dead playouts, zero denominators (random_terms) - and every row but each third one comes from an earlier round:
    its slots hold sums and counts already and the columns reach them through a permuted `slot`."""
    rng = np.random.default_rng(seed)
    terms = HR.random_terms(rng, (n, k, R))
    slot = None if identity else np.stack([rng.permutation(m)[:k] for _ in range(n)]).astype(np.int32)
    cand0 = rng.integers(0, 2000, (n, m)).astype(np.int64)
    prior = rng.normal(size=(n, m)) * 3
    count = rng.integers(0, 4, (n, m)).astype(np.int32)
    count[::3] = 0
    total = rng.uniform(-1.5, 2.0, (n, m)) * count
    for r in range(n):
        col = (lambda c: c) if slot is None else (lambda c, r=r: int(slot[r, c]))
        if r % 5 == 1:
            terms[r, :, :, 0] = 1
        elif r % 5 == 2:
            terms[r] = 0
        else:
            for c in range(k):
                what = rng.integers(0, 6)
                if what == 0:
                    terms[r, c] = 0
                elif what == 1:
                    cand0[r, col(c)] = HR.NONE
                    if rng.integers(0, 2):
                        terms[r, c] = 0
                elif what == 2 and c + 1 < k:                    # this column and the next: equal keys
                    terms[r, c + 1] = terms[r, c]
                    for a in (prior, total, count):
                        a[r, col(c + 1)] = a[r, col(c)]
        if r % 4 == 3:
            cand0[r, rng.integers(0, m)] = HR.PASS
    return terms, slot, cand0, prior, total, count


HALVE_SHAPES = [(k, -(-k // 2)) for k in (1, 2, 3, 63, 64)] + [(5, 5)]


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("k,k_next", HALVE_SHAPES)
@pytest.mark.parametrize("identity", [False, True], ids=["permuted", "identity"])
def test_halve_equals_the_restatement_bit_for_bit(identity, k, k_next, R, n):
    import torch
    from generalsreinforcementlearning_amd import _lib as lib
    m = k if identity else 64
    terms, slot, cand0, prior, total, count = _halve_case(n, k, R, m, identity, seed=1000 * k + 10 * R + n)
    want_total, want_count = total.copy(), count.copy()
    want_slot, want_cand = HR.halve(terms, slot, cand0, prior, want_total, want_count, k_next, WEIGHTS, C_VISIT, C_SCALE)
    assert (want_count != count).any() or not terms[..., 0].any()
    pad = 16                                                     # sentinels past every buffer the kernel writes
    d_total = _cuda(np.concatenate([total.ravel(), np.full(pad, SENTINEL, np.float64)]))
    d_count = _cuda(np.concatenate([count.ravel(), np.full(pad, SENTINEL, np.int32)]))
    d_slot = torch.full((n * k_next + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    d_cand = torch.full((n * k_next + pad,), SENTINEL, dtype=torch.int64, device="cuda")
    d_terms, d_in_slot, d_cand0, d_prior = _cuda(terms), None if slot is None else _cuda(slot), _cuda(cand0), _cuda(prior)
    q_lo, q_inv = HR.q_range(**WEIGHTS)
    a = lib.SearchHalveArgs(n=n, m=m, k=k, replicas=R, k_next=k_next, reserved=0, terms=d_terms.data_ptr(),
                            slot=None if slot is None else d_in_slot.data_ptr(), candidates0=d_cand0.data_ptr(),
                            prior_key=d_prior.data_ptr(), q_lo=q_lo, q_inv_range=q_inv, c_visit=C_VISIT, c_scale=C_SCALE,
                            sum=d_total.data_ptr(), count=d_count.data_ptr(), next_slot=d_slot.data_ptr(),
                            next_candidates=d_cand.data_ptr(), **WEIGHTS)
    lib.check(lib.load().gvec_search_halve(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a)), "gvec_search_halve")
    got_total, got_count, got_slot, got_cand = (t.cpu().numpy() for t in (d_total, d_count, d_slot, d_cand))
    for name, got in (("sum", got_total), ("count", got_count), ("next_slot", got_slot), ("next_candidates", got_cand)):
        assert (got[-pad:] == SENTINEL).all(), f"{name}: written past its end"
    assert np.array_equal(got_count[:-pad].reshape(n, m), want_count)
    assert np.array_equal(got_total[:-pad].view(np.int64).reshape(n, m), want_total.view(np.int64))   # untouched slots included
    assert np.array_equal(got_slot[:-pad].reshape(n, k_next), want_slot)
    assert np.array_equal(got_cand[:-pad].reshape(n, k_next), want_cand)


# ---- improved_policy: against float64, the bound measured on the case's own inputs --------------------------------------------
def _policy_case(n, A, m, seed, with_logits=True):
    """Rows by r % 9: 0 all legal, 1 about 2 % legal, 2 one legal, 3 none legal, 4 nothing visited, 5 a visited PASS, 6 a
    visited candidate outside the mask, 7 and 8 ordinary (about half legal)."""
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(n, A)) * 2).astype(np.float32) if with_logits else None
    mask = rng.random((n, A)) < 0.5
    cand = np.full((n, m), HR.NONE, np.int64)
    count = rng.integers(0, 9, (n, m)).astype(np.int32)
    for r in range(n):
        kind = r % 9
        if kind == 0:
            mask[r] = True
        elif kind == 1:
            mask[r] = rng.random(A) < 0.02
            mask[r, rng.integers(0, A)] = True
        elif kind == 2:
            mask[r] = False
            mask[r, rng.integers(0, A)] = True
        elif kind == 3:
            mask[r] = False
        legal = np.flatnonzero(mask[r])
        pick = rng.permutation(legal)[:m]
        cand[r, :len(pick)] = pick
        if kind == 4:
            count[r] = 0
        elif kind == 5:
            cand[r, 0], count[r, 0] = HR.PASS, 3
        elif kind == 6:
            outside = np.flatnonzero(~mask[r])
            if len(outside):
                cand[r, m - 1], count[r, m - 1] = outside[0], 8      # it carries the row's largest count: nmax sees it, V does not
    total = rng.uniform(-1.5, 2.0, (n, m)) * count
    value = rng.uniform(-1, 1, n).astype(np.float32)
    return logits, mask, cand, total, count, value


def _torch_policy(logits, legal, cand, total, count, value, q_lo, q_inv, c_visit, c_scale):
    """the definition in torch float32 on whatever device holds the inputs: what float32 costs on these inputs"""
    import torch
    n, A = legal.shape
    dev, f32 = legal.device, torch.float32
    ninf = torch.full((), -float("inf"), dtype=f32, device=dev)
    zero = torch.zeros((), dtype=f32, device=dev)
    x = torch.where(legal, logits if logits is not None else zero, ninf)
    in_row = (count > 0) & (cand >= 0) & (cand < A)
    ai = torch.where(in_row, cand, torch.zeros_like(cand))
    xa = torch.where(in_row, x.gather(1, ai), ninf)
    vis = xa > ninf
    q = torch.where(vis, (total / count.clamp(min=1).to(torch.float64)).to(f32), zero)
    vtop = xa.max(dim=1, keepdim=True).values
    w = torch.where(vis, torch.exp(xa - torch.where(torch.isinf(vtop), zero, vtop)), zero)
    den, num = w.sum(1), (w * q).sum(1)
    N = torch.where(vis, count, torch.zeros_like(count)).sum(1).to(f32)
    has = N > 0
    vq = num / torch.where(has, den, torch.ones_like(den))
    val = value if value is not None else torch.zeros(n, dtype=f32, device=dev)
    vmix = torch.where(has, (val + N * vq) / (1 + N) if value is not None else vq, val)
    scale = ((c_visit + count.max(dim=1).values.to(torch.float64)) * c_scale).to(f32)
    lo, inv = float(np.float32(q_lo)), float(np.float32(q_inv))
    shift = torch.where(has, scale * ((vmix - lo) * inv), zero)
    y = torch.cat([x + shift[:, None], torch.zeros((n, 1), dtype=f32, device=dev)], dim=1)
    ya = xa + scale[:, None] * ((q - lo) * inv)
    y.scatter_(1, torch.where(vis, ai, torch.full_like(ai, A)), ya)
    y = y[:, :A]
    top = y.max(dim=1, keepdim=True).values
    e = torch.where(legal, torch.exp(y - torch.where(torch.isinf(top), zero, top)), zero)
    z = e.sum(1, keepdim=True)
    return e / torch.where(z > 0, z, torch.ones_like(z)), vmix


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("A", [5, 64, 65, 1125, 2000, 5120])
@pytest.mark.parametrize("form", ["value", "no_value", "no_logits"])
def test_improved_policy_stays_within_the_measured_float32_bound(form, A, n):
    import torch
    from generalsreinforcementlearning_amd import _lib as lib
    m = min(16, A)
    logits, mask, cand, total, count, value = _policy_case(n, A, m, seed=7 * A + n, with_logits=form != "no_logits")
    if form != "value":
        value = None
    want, want_v = HR.improved_policy(logits, mask, cand, total, count, value, WEIGHTS, C_VISIT, C_SCALE)
    q_lo, q_inv = HR.q_range(**WEIGHTS)
    d = dict(logits=None if logits is None else _cuda(logits), legal=_cuda(mask), cand=_cuda(cand), total=_cuda(total), count=_cuda(count),
             value=None if value is None else _cuda(value))
    t32, v32 = _torch_policy(q_lo=q_lo, q_inv=q_inv, c_visit=C_VISIT, c_scale=C_SCALE, **d)
    err32 = np.abs(t32.double().cpu().numpy() - want).max()
    verr32 = np.abs(v32.double().cpu().numpy() - want_v).max()
    pad = 16
    target = torch.full((n * A + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    v_mix = torch.full((n + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    mask8 = d["legal"].to(torch.uint8)
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    a = lib.SearchPolicyArgs(n=n, num_actions=A, m=m, reserved=0, logits=ptr(d["logits"]), mask=mask8.data_ptr(),
                             candidates0=d["cand"].data_ptr(), sum=d["total"].data_ptr(), count=d["count"].data_ptr(), value=ptr(d["value"]),
                             q_lo=q_lo, q_inv_range=q_inv, c_visit=C_VISIT, c_scale=C_SCALE, target=target.data_ptr(), v_mix=v_mix.data_ptr())
    lib.check(lib.load().gvec_search_improved_policy(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a)),
              "gvec_search_improved_policy")
    got_all, got_v_all = target.cpu().numpy(), v_mix.cpu().numpy()
    assert (got_all[-pad:] == SENTINEL).all() and (got_v_all[-pad:] == SENTINEL).all()
    got, got_v = got_all[:-pad].reshape(n, A).astype(np.float64), got_v_all[:-pad].astype(np.float64)
    err, verr = np.abs(got - want).max(), np.abs(got_v - want_v).max()
    bound, vbound = max(4 * err32, 1e-6), max(4 * verr32, 1e-6)
    print(f"improved_policy {form} A={A} n={n}: kernel {err:.3e} (torch float32 {err32:.3e}), v_mix {verr:.3e} ({verr32:.3e})")
    assert np.isfinite(got).all() and np.isfinite(got_v).all()
    assert err <= bound, (err, err32)
    assert verr <= vbound, (verr, verr32)
    # exactly: zeros outside the mask and on dead rows; a row with nothing visited is the prior and hands the value through
    assert (got[~mask] == 0).all() and (got[~mask.any(1)] == 0).all()
    live = mask.any(1)
    assert np.abs(got[live].sum(1) - 1).max() < 1e-5
    nothing = live & ~((count > 0) & (cand >= 0)).any(1)
    for r in np.flatnonzero(nothing):
        x = np.zeros(A) if logits is None else logits[r].astype(np.float64)
        e = np.where(mask[r], np.exp(x - x[mask[r]].max()), 0.0)
        assert np.abs(got[r] - e / e.sum()).max() <= bound
    quiet = ~((count > 0) & (cand >= 0) & np.take_along_axis(np.concatenate([mask, np.zeros((n, 1), bool)], 1), np.where(cand >= 0, cand, A), 1)).any(1)
    assert np.array_equal(got_v[quiet], (np.zeros(n) if value is None else value.astype(np.float64))[quiet])


# ---- end to end -------------------------------------------------------------------------------------------------------------
M, BUDGET, DEPTH, SEED = 8, 32, 4, 41


def _roots(W, Hh, B=6, turns=12):
    """an engine of B generated two-player boards under fog, `turns` agent turns old"""
    import generalsreinforcementlearning_amd as g
    eng = g.VecEngine(B, W, Hh, 2, fog_of_war=True)
    eng.reset_generated(17)
    eng.rollout(turns, 5, fused=True)
    return eng


def _root_rows(eng, W, Hh):
    """(players int32 [B], mask bool [B, 5 W H]): seats alternate; the seat's accepted full moves"""
    st = eng.game_state()
    players = (np.arange(eng.B) % 2).astype(np.int32)
    mask = np.zeros((eng.B, 5 * W * Hh), bool)
    for i in range(eng.B):
        mask[i, SR.legal_gym_actions(st, i, int(players[i]), W * Hh, True)] = True
    return st, players, mask


def _resident_bytes(eng):
    import torch
    rec = torch.zeros(eng.B * eng.state_bytes_per_env(), dtype=torch.uint8, device="cuda")
    eng.export_records(rec.data_ptr())
    eng.synchronize()
    out = {"records": rec.cpu().numpy()}
    for name, which, per in (("header", 0, 24 * 4), ("legal", 3, eng.max_p * eng.mask_bytes), ("actions", 4, eng.max_p * 8), ("err", 5, 4)):
        buf = np.zeros(eng.B * per, np.uint8)
        assert eng.L.gvec_read_buffer(eng.h, which, 0, buf.size, buf.ctypes.data) == 0
        out[name] = buf
    return out


@pytest.mark.parametrize("rollout", ["agent", "bot"])
@pytest.mark.parametrize("W,Hh", [(5, 5), (8, 8)], ids=["5x5", "8x8"])
def test_search_equals_evaluate_driven_round_by_round(W, Hh, rollout):
    import generalsreinforcementlearning_amd as g
    eng = _roots(W, Hh)
    _, players, mask = _root_rows(eng, W, Hh)
    assert (mask.sum(1) > 0).sum() >= 3
    search = g.HalvingSearch(eng, candidates=M, budget=BUDGET, depth=DEPTH, rollout=rollout)
    cand, prior = search.propose(_cuda(mask), None, SEED)
    d_players = _cuda(players)
    out = search.search(None, d_players, cand, prior, SEED)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    cand0, prior0 = cand.cpu().numpy(), prior.cpu().numpy()

    def play(c, R, r, seed):
        ps = g.PlayoutSearch(eng, candidates=c.shape[1], replicas=R, depth=DEPTH, rollout=rollout)
        return ps.evaluate(None, d_players, _cuda(c, np.int64), seed).cpu().numpy()

    total, count, slot, action = HR.search(play, cand0, prior0, BUDGET, SEED)
    assert count.sum() > 0 and (count.max(1) > 1).any()
    assert np.array_equal(got["count"], count) and np.array_equal(got["sum"].view(np.int64), total.view(np.int64))
    assert np.array_equal(got["slot"], slot) and np.array_equal(got["action"], action)
    q = (total / np.maximum(count, 1)).astype(np.float32)
    assert np.array_equal(got["q"].view(np.int32), q.view(np.int32)) and np.array_equal(got["valid"], count > 0)
    assert np.array_equal(got["found"], count[np.arange(eng.B), slot] > 0)
    # repeating the call repeats the bits
    again = {k: v.cpu().numpy() for k, v in search.search(None, d_players, cand, prior, SEED).items()}
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    eng.close()


def test_the_roots_are_read_only():
    import generalsreinforcementlearning_amd as g
    eng, twin = _roots(8, 8), _roots(8, 8)
    st, players, mask = _root_rows(eng, 8, 8)
    eng.legal_action_mask_bits()
    twin.legal_action_mask_bits()
    before, counters = _resident_bytes(eng), eng.counters()
    search = g.HalvingSearch(eng, candidates=M, budget=BUDGET, depth=DEPTH)
    cand, prior = search.propose(_cuda(mask), None, SEED)
    out = search.search(None, _cuda(players), cand, prior, SEED)
    assert int(out["count"].sum()) > 0
    after = _resident_bytes(eng)
    for k in before:
        assert np.array_equal(before[k], after[k]), f"the search changed the handle's {k}"
    assert eng.counters() == counters
    acts = eng.agent_actions(31)
    assert np.array_equal(acts, twin.agent_actions(31))
    (e1, m1), (e2, m2) = eng.step(acts, want_mask=True), twin.step(acts, want_mask=True)
    assert np.array_equal(e1, e2) and np.array_equal(m1, m2)
    a, b = eng.game_state(), twin.game_state()
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    assert eng.counters() == twin.counters()
    eng.close()
    twin.close()


def test_the_capture_of_the_general_survives_every_round():
    """tests/test_hip_search.py's position: 5x5, seat 0 holds 50 armies next to seat 1's general, the agent mix is "never
    move".  Of seat 0's seven legal actions exactly one wins, on the playout's first turn, in every playout; no other action's
    playout is won (checked on the terms).  A won playout scores 1, any other at most 0.5: sigma differs by at least
    (c_visit + 1) / 4 = 50.25 with c_visit = 200, more than two Gumbel draws from 32-bit uniforms can (22.2 + 3.1)."""
    import torch
    import _oracle as O
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    W = H_ = 5
    env = GeneralsSelfPlayVecEnv(2, board_width=W, board_height=H_, max_players=2, device_outputs=True, board_pool=4)
    env.reset()
    tiles = [dict(x=0, y=0, owner=0, army=5, type=1), dict(x=4, y=4, owner=1, army=2, type=1), dict(x=3, y=4, owner=0, army=50)]
    army, owner, typ = O.planes_from_tiles(W, H_, tiles)
    env.engine.reset(np.stack([army] * 2), np.stack([owner] * 2), np.stack([typ] * 2))
    env.engine.set_agent_mix(65536, 0)
    st = env.engine.game_state()
    capture = (4 * W + 3) * 5 + 1
    mask = np.zeros((4, W * H_ * 5), bool)
    for r in range(4):
        for a in range(W * H_ * 5):
            mask[r, a] = SR.decode_candidate(st, r // 2, r % 2, a, W * H_, True) is not None or \
                (a % 5 == 4 and any(SR.decode_candidate(st, r // 2, r % 2, a - 4 + d, W * H_, True) is not None for d in range(4)))
    assert mask[0].sum() == 7 and mask[0, capture]
    search = g.HalvingSearch(env, candidates=8, budget=32, depth=5, c_visit=200.0)
    actions, info = search.act(torch.from_numpy(mask).cuda(), seed=3)
    cand, count, q, slot = (info[k].cpu().numpy() for k in ("candidates", "count", "q", "slot"))
    # the premise, on the terms: every round's seed, all eight candidates at once
    for r, (K, R) in enumerate(search.schedule):
        ps = g.PlayoutSearch(env, candidates=8, replicas=R, depth=5)
        ids = search._rounds[0]._rows_to_ids(4, None)
        terms = ps.evaluate(ids[0], ids[1], info["candidates"], search.round_seed(3, r)).cpu().numpy()
        for row in (0, 2):
            k = int(np.flatnonzero(cand[row] == capture)[0])
            assert terms[row, k, :, 0].all() and terms[row, k, :, 3].all(), "the premise failed: a playout of the capture is not won"
            assert not terms[row, [j for j in range(8) if j != k]][..., 3].any(), "the premise failed: another move's playout is won"
    spent = sum(R for _, R in search.schedule)
    for row in (0, 2):
        k = int(np.flatnonzero(cand[row] == capture)[0])
        assert count[row, k] == spent and slot[row] == k and q[row, k] == 1.0
        assert sorted(cand[row][count[row] > 0].tolist()) == np.flatnonzero(mask[0]).tolist()
    assert actions.cpu().tolist()[0::2] == [capture, capture]
    # the policy target prefers it, sums to one and stays on the mask
    d_mask = torch.from_numpy(mask).cuda()
    target, v_mix = search.policy_target(None, d_mask, info)
    t = target.cpu().numpy()
    assert int(t[0].argmax()) == capture and np.abs(t.sum(1) - 1).max() < 1e-5 and (t[~mask] == 0).all()
    assert np.isfinite(v_mix.cpu().numpy()).all()
    env.close()


def test_an_arena_entrant_plays_legal_actions():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(16, board_width=8, board_height=8, max_players=2, device_outputs=True, board_pool=32)
    search = g.HalvingSearch(env, candidates=4, budget=8, depth=4)
    policy = g.playout_policy(search, seed=1)
    arena = g.Arena(env, [policy, g.random_policy(seed=2)])
    invalid = torch.zeros((16, 2), dtype=torch.int32, device="cuda")
    for _ in range(20):
        out = arena.step()
        invalid += out[4]["invalid"].to(torch.int32)
    assert int(invalid.sum()) == 0 and policy._calls == 20
    env.close()
