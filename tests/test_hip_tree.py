"""The tree search on the GPU (include/generals_vec.h "tree search below the root").
gvec_search_expand: its terms against gvec_search_playouts / _bot bit for bit, its stored boards against the CPU oracle's state
after the playout's first step - every compiled variant, the roots whose games end, the rare state forms - and against the
composition of existing calls on the device.  gvec_tree_select against the plain-Python restatement on inputs whose every
decision is an exact tie or clear of 1e-9; gvec_tree_backup against it bit for bit.  TreeSearch end to end on small engines:
equal to the same loop with the restatements doing select and backup, repeatable, read-only on its roots, and right in a
position whose answer is two moves deep."""
import ctypes as C

import numpy as np
import pytest

import _halving_reference as HR
import _harness as H
import _oracle as O
import _search_reference as SR
import _state_forms as SF
import _tree_reference as TR
from _bot_reference import bot_actions

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _cuda(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- gvec_search_expand ---------------------------------------------------------------------------------------------------------
def _expand(eng, players, cand, R, D, seed, bot=0, permille=0, dst=None, child_envs=None, env_ids=None):
    """(terms [n, K, R, 8], status [n, K]) on the host; status starts as the sentinel"""
    import torch
    from generalsreinforcementlearning_amd.search import search_expand_device
    cand = np.asarray(cand, np.int64)
    n, K = cand.shape
    d_cand, d_players = _cuda(cand, np.int64), _cuda(players, np.int32)
    d_ids = None if env_ids is None else _cuda(env_ids, np.int32)
    d_child = None if child_envs is None else _cuda(child_envs, np.int32)
    terms = torch.full((n, K, R, 8), SENTINEL, dtype=torch.int32, device="cuda")
    status = torch.full((n, K), SENTINEL, dtype=torch.int32, device="cuda")
    search_expand_device(eng, n, d_cand.data_ptr(), d_players.data_ptr(), terms.data_ptr(), K, R, D, seed,
                         None if d_ids is None else d_ids.data_ptr(), bot, permille, dst=dst,
                         child_envs_ptr=None if d_child is None else d_child.data_ptr(), status_ptr=status.data_ptr())
    eng.synchronize()
    return terms.cpu().numpy(), status.cpu().numpy()


def _playouts(eng, players, cand, R, D, seed, bot=0, permille=0):
    import torch
    cand = np.asarray(cand, np.int64)
    n, K = cand.shape
    d_cand, d_players = _cuda(cand, np.int64), _cuda(players, np.int32)
    terms = torch.full((n, K, R, 8), SENTINEL, dtype=torch.int32, device="cuda")
    eng.search_playouts_device(n, d_cand.data_ptr(), d_players.data_ptr(), terms.data_ptr(), K, R, D, seed, None, bot, permille)
    eng.synchronize()
    return terms.cpu().numpy()


def _resident_bytes(eng):
    """test_hip_search.py's: the canonical records of every env and the raw header, legal-mask, action and err buffers"""
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


def _env_records(eng):
    """uint8 [B, bytes per env]: every env's canonical record (header with the lifetime counters, planes, armies) on its own"""
    import torch
    per = eng.state_bytes_per_env()
    rec = torch.zeros((eng.B, per), dtype=torch.uint8, device="cuda")
    for e in range(eng.B):
        eng.export_records(rec[e].data_ptr(), e, 1)
    eng.synchronize()
    return rec.cpu().numpy()


def _twins(mw, mh, maxp, sizes, fog=True, board_seed=3):
    import generalsreinforcementlearning_amd as g
    boards = H.gen_boards(board_seed, sizes, mw, mh)
    eng = g.VecEngine(len(sizes), mw, mh, maxp, fog_of_war=fog)
    ora = O.OracleBatch(len(sizes), mw, mh, maxp, fog=fog)
    eng.reset(*boards)
    ora.reset(*boards)
    return eng, ora


def _scratch(n, mw, mh, maxp, fog=True, played=3):
    """an engine of n envs that hold games of their own, a few turns old: what expand must overwrite completely"""
    import generalsreinforcementlearning_amd as g
    eng = g.VecEngine(n, mw, mh, maxp, fog_of_war=fog)
    eng.reset(*H.gen_boards(17, [(mw, mh, 2)] * n, mw, mh))
    if played:
        eng.rollout(played, 77)
    return eng


def _candidates(st, players, stride, fog, with_half=False):
    """test_hip_search.py's [n, 5]: three accepted moves (first, middle - with_half: as a half move -, last), the pass, padding"""
    n = len(players)
    cand = np.full((n, 5), SR.NONE, np.int64)
    for i in range(n):
        legal = SR.legal_gym_actions(st, i, int(players[i]), stride, fog)
        if legal:
            mid = legal[len(legal) // 2]
            cand[i, :3] = [legal[0], mid // 5 * 5 + 4 if with_half else mid, legal[-1]]
        cand[i, 3] = SR.PASS
    return cand


def _oracle_children(st, players, cand, R, seed, mw, mh, maxp, fog, bot=0, permille=0, mix=(6554, 19661)):
    """(plan, the oracle's state of every playout after its first step): gvec_search_playouts' definition up to that step"""
    plan = SR.Plan(st, None, players, cand, R, mw, mh, maxp, fog)
    st0 = SR.repeat_state(st, plan.src)
    ora = O.OracleBatch(plan.V, mw, mh, maxp, fog=fog)
    ora.set_agent_mix(*mix)
    ora.reset(st0["army"], st0["owner"], st0["type"], st0["width"], st0["height"], st0["players"])
    ora.write_state({k: st0[k] for k in SR.IMPORTED})
    acts = ora.agent_actions(seed)
    if bot or permille:
        acts = bot_actions(ora.read_state(), bot, fog, seed, permille, agent=acts.copy(), out=acts, max_p=maxp)
    ora.step(plan.override(acts))
    return plan, ora.read_state()


def _check_children(eng, st, players, cand, R, D, seed, mw, mh, maxp, fog, bot=0, permille=0, mix=(6554, 19661), ctx=""):
    """expand into a scratch engine: the terms are the playout call's, every stored env is the oracle's state after the first
    step field for field, the status bits say what happened, and nothing else of the scratch engine changed.  Returns the
    oracle's children and which pairs were stored."""
    n, K = cand.shape
    plan, after = _oracle_children(st, players, cand, R, seed, mw, mh, maxp, fog, bot, permille, mix)
    first = np.arange(n * K) * R
    want, valid = SR.repeat_state(after, first), plan.valid[first]
    seat = plan.seat[first]
    dst = _scratch(n * K, mw, mh, maxp, fog)
    before, rec_before = _resident_bytes(dst), _env_records(dst)
    terms, status = _expand(eng, players, cand, R, D, seed, bot, permille, dst=dst)
    assert np.array_equal(terms, _playouts(eng, players, cand, R, D, seed, bot, permille)), f"{ctx}: terms differ from the playout call's"
    after_b, rec_after = _resident_bytes(dst), _env_records(dst)
    rows = np.flatnonzero(valid)
    assert len(rows) >= n // 2, ctx
    H.assert_states_equal(SR.repeat_state(dst.game_state(), rows), SR.repeat_state(want, rows), f"{ctx}: stored boards")
    want_status = np.where(valid, 1 | np.where(want["done"] != 0, 2, 0) | np.where(want["alive"][np.arange(n * K), seat] == 0, 4, 0), 0)
    assert np.array_equal(status.ravel(), want_status), f"{ctx}: status {status.ravel().tolist()} != {want_status.tolist()}"
    untouched = np.flatnonzero(~valid)
    assert np.array_equal(rec_before[untouched], rec_after[untouched]), f"{ctx}: an env without a stored child changed"
    assert (rec_before[rows] != rec_after[rows]).any(axis=1).all()
    hb, ha = before["header"].view(np.uint32).reshape(-1, 24), after_b["header"].view(np.uint32).reshape(-1, 24)
    assert np.array_equal(hb[untouched], ha[untouched])
    assert np.array_equal(hb[:, 21:24], ha[:, 21:24]), f"{ctx}: a destination slot's lifetime counters changed"
    assert (hb[rows, 0] != ha[rows, 0]).any() or (hb[rows, 1] != ha[rows, 1]).any()
    for k in ("legal", "actions", "err"):
        assert np.array_equal(before[k], after_b[k]), f"{ctx}: expand touched the destination's {k} buffer"
    dst.close()
    return want, valid


@pytest.mark.parametrize("maxp", [2, 4, 8])
@pytest.mark.parametrize("slots,parity", sorted(H.VARIANT_DIMS), ids=H.VARIANT_IDS)
def test_every_variant_stores_the_oracles_boards(maxp, slots, parity):
    B, R, D, seed = 4, 2, 3, 11
    mw, mh, sizes = H.variant_batch(maxp, slots, parity, B)
    eng, ora = _twins(mw, mh, maxp, sizes)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(B) + 1) % st["players"]
    cand = _candidates(st, players, mw * mh, True)
    before = _resident_bytes(eng)
    _check_children(eng, st, players, cand, R, D, seed, mw, mh, maxp, True, ctx=f"agent P{maxp} slots {slots} {parity}")
    _check_children(eng, st, players, cand, R, D, seed, mw, mh, maxp, True, bot=(1 << maxp) - 1, ctx=f"bot P{maxp} slots {slots} {parity}")
    after = _resident_bytes(eng)
    assert all(np.array_equal(before[k], after[k]) for k in before), "expand changed its roots"
    eng.close()


@pytest.mark.parametrize("bot,permille", [(0, 0), (0b11, 500)], ids=["agent", "bot_mix500"])
@pytest.mark.parametrize("fog", [False, True], ids=["nofog", "fog"])
def test_coverage_roots_store_the_oracles_boards(fog, bot, permille):
    """the 5x5 roots whose playouts are won, lost, cut short, refused, passed and padded"""
    import generalsreinforcementlearning_amd as g
    st, players, cand = SR.coverage_roots(fog)
    n = len(players)
    eng = g.VecEngine(n, SR.COVER_W, SR.COVER_H, SR.COVER_P, fog_of_war=fog)
    eng.reset(st["army"], st["owner"], st["type"], st["width"], st["height"], st["players"])
    eng.write_state({k: st[k] for k in SR.IMPORTED if k not in ("width", "height", "players")})
    H.assert_states_equal(eng.game_state(), st, "the engine did not take the roots")
    want, valid = _check_children(eng, st, players, cand, 2, 4, SR.COVER_SEARCH_SEED, SR.COVER_W, SR.COVER_H, SR.COVER_P, fog, bot, permille,
                                  ctx=f"fog {fog} bot {bot:#b}/{permille}")
    assert (want["done"][valid] != 0).any() and (want["done"][valid] == 0).any() and (~valid).any()
    eng.close()


def test_rare_state_forms_store_the_oracles_boards():
    """wide armies and lists that differ from ownership, in the roots and in the stored children"""
    B, w, h, p, R, D, seed = 36, 10, 10, 4, 1, 3, 5
    eng, ora = _twins(w, h, p, [(w, h, p if i % 2 else 3) for i in range(B)], board_seed=21)
    H.run_lockstep(eng, ora, 20, seed=4, check_every=20, want_mask=False, ctx="youth")
    SF.age_batch(eng, 7)
    SF.age_batch(ora, 7)
    H.run_lockstep(eng, ora, 12, seed=13, invalid_permille=200, check_every=12, want_mask=False, ctx="ageing")
    st = eng.game_state()
    wide, desynced = SF.wide_envs(st), SF.desynced_envs(st)
    assert wide.sum() >= 4 and desynced.sum() >= 4
    players = np.arange(B) % st["players"]
    cand = _candidates(st, players, w * h, True, with_half=True)
    for bot in (0, 0b1111):
        want, valid = _check_children(eng, st, players, cand, R, D, seed, w, h, p, True, bot=bot, ctx=f"aged roots bot {bot:#b}")
        assert SF.wide_envs(want)[valid].any() and SF.desynced_envs(want)[valid].any()
    eng.close()


@pytest.mark.parametrize("bot,permille", [(0, 0), (0b0110, 300)], ids=["agent", "two_seats_mix300"])
def test_equals_the_composition_of_existing_calls_on_the_device(bot, permille):
    """copy_envs of every root K * R times into a twin, agent_actions (+ bot_actions), the candidate, one step: env (i * K + k)
    * R of the twin is what expand stores - here through explicit child_envs, some of them -1 and out of range - and one
    further common step leaves the two equal again."""
    import generalsreinforcementlearning_amd as g
    B, R, D, seed = 6, 2, 6, 23
    mw, mh, sizes = H.variant_batch(4, 4, "odd", B)
    eng, ora = _twins(mw, mh, 4, sizes)
    H.run_lockstep(eng, ora, 40, seed=5, check_every=40, want_mask=False, ctx="roots")
    st = eng.game_state()
    players = (np.arange(B) + 1) % st["players"]
    cand = _candidates(st, players, mw * mh, True, with_half=True)
    n, K = cand.shape
    plan = SR.Plan(st, None, players, cand, R, mw, mh, 4, True)
    twin = g.VecEngine(plan.V, mw, mh, 4)
    twin.copy_envs(src_ids=plan.src.astype(np.int32), src=eng)
    acts = twin.agent_actions(seed)
    if bot or permille:
        twin.bot_actions(bot, seed, permille, actions=acts)
    twin.step(plan.override(acts))
    first = np.arange(n * K) * R
    child = first.astype(np.int32).reshape(n, K).copy()
    child[0, 0], child[1, 1], child[2, 2], child[3, 0] = -1, plan.V, 2 ** 30, -5      # nothing is stored for these four
    skipped = np.zeros((n, K), bool)
    skipped[0, 0] = skipped[1, 1] = skipped[2, 2] = skipped[3, 0] = True
    stored = (plan.valid[first].reshape(n, K)) & ~skipped
    dst = _scratch(plan.V, mw, mh, 4)
    rec_b = _env_records(dst)
    eng.legal_action_mask_bits()
    roots_before = _resident_bytes(eng)
    terms, status = _expand(eng, players, cand, R, D, seed, bot, permille, dst=dst, child_envs=child)
    assert np.array_equal(terms, _playouts(eng, players, cand, R, D, seed, bot, permille))
    assert np.array_equal(terms, _expand(eng, players, cand, R, D, seed, bot, permille)[0])          # dst NULL: the playout launch
    roots_after = _resident_bytes(eng)
    assert all(np.array_equal(roots_before[k], roots_after[k]) for k in roots_before), "expand changed its roots"
    assert np.array_equal((status & 1) != 0, stored) and not status[~plan.valid[first].reshape(n, K)].any()
    assert (status[skipped & plan.valid[first].reshape(n, K)] & 1 == 0).all()
    rows = first[stored.ravel()]
    rec_a = _env_records(dst)
    H.assert_states_equal(SR.repeat_state(dst.game_state(), rows), SR.repeat_state(twin.game_state(), rows), "stored boards")
    keep = np.ones(plan.V, bool)
    keep[rows] = False
    assert np.array_equal(rec_b[keep], rec_a[keep]), "an env without a stored child changed"
    # every later call behaves as if the env had always held that state: one further common step
    nxt = twin.agent_actions(99)
    (e1, m1), (e2, m2) = dst.step(nxt, want_mask=True), twin.step(nxt, want_mask=True)
    assert np.array_equal(e1[rows], e2[rows]) and np.array_equal(m1[rows], m2[rows])
    H.assert_states_equal(SR.repeat_state(dst.game_state(), rows), SR.repeat_state(twin.game_state(), rows), "the step after")
    # the device agent draws from the stored state too (its legal-mask buffer is refreshed)
    assert np.array_equal(dst.agent_actions(5)[rows], twin.agent_actions(5)[rows])
    for e in (eng, twin, dst):
        e.close()


def test_destination_handles():
    """a mismatched dst is refused with the field named; dst == h with child envs that are no roots works"""
    import generalsreinforcementlearning_amd as g
    B, R, D, seed = 4, 2, 3, 7
    eng, ora = _twins(8, 8, 2, [(8, 8, 2)] * (3 * B))
    H.run_lockstep(eng, ora, 30, seed=5, check_every=30, want_mask=False, ctx="roots")
    st = eng.game_state()
    roots = SR.repeat_state(st, np.arange(B))
    players = np.arange(B) % 2
    cand = _candidates(roots, players, 64, True)[:, :2]
    for other, field in ((g.VecEngine(4, 8, 9, 2), "max_height"), (g.VecEngine(4, 8, 8, 4), "max_players"),
                         (g.VecEngine(4, 8, 8, 2, production=(1, 2, 1)), "prod_city"),
                         (g.VecEngine(4, 8, 8, 2, normal_growth_interval=10), "normal_growth_interval")):
        with pytest.raises(g.GvecError, match=f"gvec_search_expand: the handles differ in {field}"):
            _expand(eng, players, cand, R, D, seed, dst=other)
        other.close()
    # dst == h: roots are envs 0 .. B-1, the children go to envs B .. 3B-1
    plan, after = _oracle_children(roots, players, cand, R, seed, 8, 8, 2, True)
    first = np.arange(B * 2) * R
    child = (B + np.arange(B * 2)).astype(np.int32).reshape(B, 2)
    terms, status = _expand(eng, players, cand, R, D, seed, dst=eng, child_envs=child, env_ids=np.arange(B))
    ok = plan.valid[first]
    assert np.array_equal(terms, _playouts(eng, players, cand, R, D, seed)) and np.array_equal((status & 1).ravel() != 0, ok) and ok.sum() >= B
    got = eng.game_state()
    H.assert_states_equal(SR.repeat_state(got, child.ravel()[ok]), SR.repeat_state(after, first[ok]), "dst == h")
    H.assert_states_equal(SR.repeat_state(got, np.arange(B)), roots, "the roots of dst == h")
    eng.close()


# ---- synthetic trees --------------------------------------------------------------------------------------------------------
def _random_tree(rng, nodes, n, C, spare=0):
    """Trees of up to `nodes` nodes a row (ids below nodes; `spare` more are left unused behind them) with chains down to depth
    6, dead edges, NONE padding, terminal nodes, nodes without an open slot, fresh nodes (nothing visited) and nodes whose
    logits are all equal - a fresh one of those is an exact tie.  Unused nodes hold sentinels."""
    T = TR.new_tree(nodes + spare, n, C)
    for k in ("child_count", "node_status", "node_parent", "node_slot"):
        T[k][1:] = SENTINEL
    T["child_sum"][1:], T["node_value"][1:], T["child_logit"][1:] = SENTINEL, SENTINEL, SENTINEL
    for r in range(n):
        depth, live = {0: 0}, [0]

        def fill(v, real):
            T["child_action"][v, r] = TR.NONE
            T["child_action"][v, r, :real] = rng.integers(0, 2000, real)
            T["child_node"][v, r] = np.where(rng.random(C) < 0.1, TR.DEAD, TR.NOT_EXPANDED)
            T["child_count"][v, r], T["child_sum"][v, r] = 0, 0.0
            T["child_logit"][v, r] = 1.5 if v % 3 == 0 else (rng.normal(size=C) * 2).astype(np.float32)
            T["node_value"][v, r] = rng.uniform(-1, 1)

        fill(0, C if r % 4 else max(1, C - 2))
        T["node_status"][0, r], T["node_parent"][0, r], T["node_slot"][0, r] = TR.IN_USE, 0, 0
        for v in range(1, nodes):
            u = live[-1] if rng.random() < 0.5 else live[rng.integers(0, len(live))]
            free = np.flatnonzero((T["child_action"][u, r] != TR.NONE) & (T["child_node"][u, r] == TR.NOT_EXPANDED))
            if depth[u] >= 6 or not len(free):
                continue
            s = int(free[rng.integers(0, len(free))])
            kind = rng.integers(0, 8)
            fill(v, 0 if kind == 0 else min(C, int(rng.choice([1, 2, 4, C, rng.integers(1, C + 1)]))))
            T["node_status"][v, r] = TR.IN_USE | (TR.TERMINAL if kind == 1 else 0)
            T["node_parent"][v, r], T["node_slot"][v, r] = u, s
            T["child_node"][u, r, s] = v
            cnt = int(rng.integers(1, 6))
            T["child_count"][u, r, s], T["child_sum"][u, r, s] = cnt, rng.uniform(-1, 1) * cnt
            depth[v] = depth[u] + 1
            if kind > 1:
                live.append(v)
    return T


def _device_tree(T, pad=16):
    """(device tensors with `pad` sentinels past every array, a gvec_tree over them)"""
    from generalsreinforcementlearning_amd import _lib as lib
    nodes, n, C = T["child_action"].shape
    dev = {k: _cuda(np.concatenate([v.ravel(), np.full(pad, SENTINEL, v.dtype)])) for k, v in T.items()}
    return dev, lib.Tree(n=n, nodes=nodes, num_slots=C, reserved=0, **{k: v.data_ptr() for k, v in dev.items()})


def _read_tree(dev, T, pad=16):
    out = {}
    for k, v in dev.items():
        a = v.cpu().numpy()
        assert (a[-pad:] == SENTINEL).all(), f"{k}: written past its end"
        out[k] = a[:-pad].reshape(T[k].shape)
    return out


WEIGHTS = dict(win=2.0, loss=-1.5, land=0.25, army=1.0)
C_VISIT, C_SCALE = 50.0, 1.0
SELECT_SHAPES = [(1, 1), (2, 1), (5, 1), (5, 3), (63, 1), (63, 3), (64, 1), (64, 3), (64, 64)]


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("C_,k", SELECT_SHAPES)
def test_select_equals_the_restatement(C_, k, n):
    import torch
    from generalsreinforcementlearning_amd import _lib as lib
    rng = np.random.default_rng(7000 + 100 * C_ + 10 * k + n)
    T = _random_tree(rng, 24, n, C_)
    slot = None if k == C_ and n % 2 else np.stack([rng.permutation(C_)[:k] for _ in range(n)]).astype(np.int32)
    want = TR.select(T, slot, k, WEIGHTS, C_VISIT, C_SCALE)
    gaps = np.array(want[4])
    assert ((gaps == 0) | (gaps > 1e-9)).all(), "a decision of this input is neither a tie nor clear: draw another seed"
    if n == 257 and k == 64:
        assert sorted(set(want[3].ravel().tolist())) == list(range(7))          # leaves at every depth from 0 to 6
    if n == 257 and C_ >= 5:
        assert want[3].max() >= 3 and (want[1] < 0).any() and (want[1] >= 0).any() and (gaps == 0).any() and (gaps > 1e-9).any()
    before = {k_: v.copy() for k_, v in T.items()}
    dev, tree = _device_tree(T)
    pad = 16
    outs = [torch.full((n * k + pad,), SENTINEL, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64, torch.int32)]
    d_slot = None if slot is None else _cuda(slot)
    q_lo, q_inv = HR.q_range(**WEIGHTS)
    a = lib.TreeSelectArgs(tree=tree, k=k, reserved=0, slot=None if slot is None else d_slot.data_ptr(), q_lo=q_lo, q_inv_range=q_inv,
                           c_visit=C_VISIT, c_scale=C_SCALE, leaf_node=outs[0].data_ptr(), leaf_slot=outs[1].data_ptr(),
                           leaf_action=outs[2].data_ptr(), leaf_depth=outs[3].data_ptr())
    lib.check(lib.load().gvec_tree_select(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a)), "gvec_tree_select")
    for name, o, w in zip(("leaf_node", "leaf_slot", "leaf_action", "leaf_depth"), outs, want):
        got = o.cpu().numpy()
        assert (got[-pad:] == SENTINEL).all(), f"{name}: written past its end"
        assert np.array_equal(got[:-pad].reshape(n, k), w), name
    after = _read_tree(dev, T)
    assert all(np.array_equal(after[k_].view(np.uint8), before[k_].view(np.uint8)) for k_ in T), "select wrote to the tree"


@pytest.mark.parametrize("with_net", [False, True], ids=["playouts", "net_value"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("n,C_,k", [(1, 1, 1), (5, 5, 3), (5, 63, 3), (257, 64, 64)])
def test_backup_equals_the_restatement_bit_for_bit(n, C_, k, R, with_net):
    import torch
    from generalsreinforcementlearning_amd import _lib as lib
    rng = np.random.default_rng(9000 + 100 * C_ + 10 * R + n)
    nodes = 24
    T = _random_tree(rng, nodes, n, C_, spare=k)
    slot = np.stack([rng.permutation(C_)[:k] for _ in range(n)]).astype(np.int32)
    leaf_node, leaf_slot, _, _, _ = TR.select(T, slot, k, WEIGHTS, C_VISIT, C_SCALE)
    terms = HR.random_terms(rng, (n, k, R))
    status = rng.integers(0, 8, (n, k)).astype(np.int32) | np.where(rng.random((n, k)) < 0.8, 1, 0).astype(np.int32)
    new_node = np.tile(nodes + np.arange(k, dtype=np.int32), (n, 1))
    net = rng.uniform(-1.5, 2.0, (n, k)).astype(np.float32) if with_net else None
    w = 0.3 if with_net else 0.0
    dev, tree = _device_tree(T)
    want = {k_: v.copy() for k_, v in T.items()}
    TR.backup(want, leaf_node, leaf_slot, new_node, terms, status, net, w, WEIGHTS)
    if n == 257:
        terminal_revisit = (leaf_slot < 0) & (leaf_node > 0) & ((T["node_status"][leaf_node, np.arange(n)[:, None]] & TR.TERMINAL) != 0)
        assert terminal_revisit.any() and (want["child_node"] == TR.DEAD).sum() > (T["child_node"] == TR.DEAD).sum()
        assert (want["node_status"][nodes:] == TR.IN_USE).any() and (want["node_status"][nodes:] == (TR.IN_USE | TR.TERMINAL)).any()
    d = [_cuda(x) for x in (leaf_node, leaf_slot, new_node, terms, status)]
    d_net = None if net is None else _cuda(net)
    a = lib.TreeBackupArgs(tree=tree, k=k, replicas=R, leaf_node=d[0].data_ptr(), leaf_slot=d[1].data_ptr(), new_node=d[2].data_ptr(),
                           terms=d[3].data_ptr(), status=d[4].data_ptr(), net_value=None if net is None else d_net.data_ptr(),
                           value_weight=w, **WEIGHTS)
    lib.check(lib.load().gvec_tree_backup(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a)), "gvec_tree_backup")
    got = _read_tree(dev, T)
    for k_ in T:
        assert np.array_equal(got[k_].view(np.uint8), want[k_].view(np.uint8)), k_     # bit for bit, sentinels in unused nodes included


# ---- TreeSearch end to end --------------------------------------------------------------------------------------------------
def _gym_mask(st, rows_env, rows_seat, W, Hh, fog):
    stride = W * Hh
    mask = np.zeros((len(rows_env), stride * 5), bool)
    for r, (e, p) in enumerate(zip(rows_env, rows_seat)):
        for t in range(stride):
            ok = [SR.decode_candidate(st, e, p, t * 5 + d, stride, fog) is not None for d in range(4)]
            mask[r, t * 5:t * 5 + 4] = ok
            mask[r, t * 5 + 4] = any(ok)
    return mask


def _aged_env(W, B, turns, seed):
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(B, board_width=W, board_height=W, max_players=2, device_outputs=True, board_pool=2 * B, seed=seed)
    env.reset()
    env.engine.rollout(turns, seed + 1)
    st = env.engine.game_state()
    rows_env, rows_seat = np.repeat(np.arange(B), 2), np.tile(np.arange(2), B)
    return env, st, _gym_mask(st, rows_env, rows_seat, W, W, True)


def _restated_search(s, env_ids, players, cand, prior, seed, weights):
    """TreeSearch.search's loop with the restatements doing select, backup and the ranking; the device does expand, observe,
    the priors and the copies"""
    import torch
    n = cand.shape[0]
    tree, key = s.start(env_ids, players, cand, prior)
    T = {k: v.cpu().numpy().copy() for k, v in tree.items()}
    key = key.cpu().numpy()
    slot = np.tile(np.arange(s.m, dtype=np.int32), (n, 1))
    wave, used, gaps = 0, 1, []
    for K, R in s.schedule:
        for _ in range(R):
            wave_seed = s.round_seed(seed, wave)
            leaf_node, leaf_slot, leaf_action, leaf_depth, g = TR.select(T, slot, K, weights, s.c_visit, s.c_scale)
            gaps += g
            terms, status = s.expand(n, players, _cuda(leaf_node), _cuda(leaf_action), wave_seed)
            obs, mask = s.observe(n, K, players, _cuda(leaf_depth.astype(np.int64) + 1))
            slots, logits, value = s.priors(obs, mask, wave_seed)
            new_node = np.tile(used + np.arange(K, dtype=np.int32), (n, 1))
            for r in range(n):
                for c in range(K):
                    T["child_action"][new_node[r, c], r] = slots[r * K + c].cpu().numpy()
                    T["child_logit"][new_node[r, c], r] = logits[r * K + c].cpu().numpy()
            TR.backup(T, leaf_node, leaf_slot, new_node, terms.cpu().numpy(), status.cpu().numpy(), None, 0.0, weights)
            s.keep(n, _cuda(new_node))
            wave, used = wave + 1, used + K
        zeros = np.zeros((n, K, 1, 8), np.int32)
        slot, _ = HR.halve(zeros, slot, T["child_action"][0], key, T["child_sum"][0], T["child_count"][0], (K + 1) // 2, weights,
                           s.c_visit, s.c_scale)
    return T, slot[:, 0], gaps


@pytest.mark.parametrize("rollout", ["agent", "bot"])
@pytest.mark.parametrize("W", [5, 8])
def test_search_equals_the_loop_with_the_restatements(W, rollout):
    import torch
    import generalsreinforcementlearning_amd as g
    B = 3
    env, st, mask = _aged_env(W, B, 30, seed=5 + W)
    twin, _, _ = _aged_env(W, B, 30, seed=5 + W)                              # the same history, never searched
    H.assert_states_equal(env.engine.game_state(), twin.engine.game_state(), "twins")
    bot = dict(rollout="bot", bot_random_permille=200) if rollout == "bot" else {}
    s = g.TreeSearch(env, candidates=4, simulations=24, depth=4, replicas=2, **bot)
    assert s.schedule == [(4, 3), (2, 6)] and s.nodes == 25
    d_mask = torch.from_numpy(mask).cuda()
    env.engine.legal_action_mask_bits()
    before = _resident_bytes(env.engine)
    actions, info = s.act(d_mask, seed=3)
    again_actions, again = s.act(d_mask, seed=3)
    after = _resident_bytes(env.engine)
    assert all(np.array_equal(before[k], after[k]) for k in before), "the search changed its root engine"
    for k in ("sum", "count", "slot", "action", "nodes_used"):
        assert torch.equal(info[k].view(torch.int64) if info[k].dtype == torch.float64 else info[k],
                           again[k].view(torch.int64) if again[k].dtype == torch.float64 else again[k]), f"{k} does not repeat"
    for k in info["tree"]:
        assert np.array_equal(info["tree"][k].cpu().numpy().view(np.uint8), again["tree"][k].cpu().numpy().view(np.uint8)), k
    assert torch.equal(actions, again_actions)
    # the loop with the restatements
    env_ids, players = s._halving._rounds[0]._rows_to_ids(2 * B, None)
    weights = dict(win=s.score.win, loss=s.score.loss, land=s.score.land, army=s.score.army)
    T, survivor, gaps = _restated_search(s, env_ids, players, info["candidates"], info["prior_key"], 3, weights)
    gaps = np.array(gaps)
    assert len(gaps) and ((gaps == 0) | (gaps > 1e-9)).all()
    tree = {k: v.cpu().numpy() for k, v in info["tree"].items()}
    assert np.array_equal(tree["child_sum"].view(np.int64), T["child_sum"].view(np.int64))               # to the bit, every node
    for k in ("child_count", "child_node", "child_action", "node_status", "node_parent", "node_slot"):
        assert np.array_equal(tree[k], T[k]), k
    assert np.array_equal(tree["node_value"].view(np.int64), T["node_value"].view(np.int64))
    assert np.array_equal(info["sum"].cpu().numpy().view(np.int64), T["child_sum"][0].view(np.int64))
    assert np.array_equal(info["count"].cpu().numpy(), T["child_count"][0])
    assert np.array_equal(info["slot"].cpu().numpy(), survivor)
    assert np.array_equal(info["nodes_used"].cpu().numpy(), (T["node_status"] & 1).sum(axis=0))
    live = mask.any(axis=1)
    assert (info["nodes_used"].cpu().numpy()[live] > 1 + s.m).all()           # nodes below the root's children
    assert (tree["child_count"][1:].sum(axis=(0, 2))[live] > 0).all()         # ... reached by visits: the walk descended
    legal = mask[np.arange(2 * B), actions.cpu().numpy()]
    assert legal[live].all()
    # the policy target over the root's slots
    target, v_mix = s.policy_target(None, d_mask, info)
    sums = target.double().sum(dim=1).cpu().numpy()
    assert np.abs(sums[live] - 1.0).max() < 1e-5 and ((target > 0).cpu().numpy() <= mask).all()
    # the root engine plays on as its twin does
    out1, out2 = env.engine.rollout(3, 41), twin.engine.rollout(3, 41)
    H.assert_states_equal(env.engine.game_state(), twin.engine.game_state(), "the turns after a search")
    assert out1 == out2
    s.close()
    env.close()
    twin.close()


def test_one_visit_per_slot_is_the_flat_search():
    """a wave over the root's own slots descends nowhere: its backed-up values are PlayoutSearch's playout means under the
    wave's seed, to the bit"""
    import torch
    import generalsreinforcementlearning_amd as g
    B, m, R = 3, 6, 3
    env, st, mask = _aged_env(8, B, 30, seed=9)
    s = g.TreeSearch(env, candidates=m, simulations=m, depth=5, replicas=R)
    flat = g.PlayoutSearch(env, candidates=m, replicas=R, depth=5)
    d_mask = torch.from_numpy(mask).cuda()
    cand, prior = s.propose(d_mask, None, seed=2)
    env_ids, players = flat._rows_to_ids(2 * B, None)
    tree, _ = s.start(env_ids, players, cand, prior)
    slot = torch.arange(m, dtype=torch.int32, device="cuda").repeat(2 * B, 1).contiguous()
    leaf_node, leaf_slot, leaf_action, leaf_depth = s.select(tree, slot)
    assert not leaf_node.any() and torch.equal(leaf_slot, slot) and torch.equal(leaf_action, cand) and not leaf_depth.any()
    terms, status = s.expand(2 * B, players, leaf_node, leaf_action, s.round_seed(2, 0))
    want_terms = flat.evaluate(env_ids, players, cand, s.round_seed(2, 0))
    assert torch.equal(terms, want_terms)
    new_node = (1 + torch.arange(m, dtype=torch.int32, device="cuda")).repeat(2 * B, 1).contiguous()
    s.backup(tree, leaf_node, leaf_slot, new_node, terms, status)
    t = want_terms.cpu().numpy()
    scores = HR.playout_scores(t)
    want = np.zeros((2 * B, m))
    for r in range(2 * B):
        for c in range(m):
            total, cnt = 0.0, 0
            for j in range(R):
                if t[r, c, j, 0]:
                    total, cnt = total + float(scores[r, c, j]), cnt + 1
            want[r, c] = total / cnt if cnt else 0.0
    got_sum, got_cnt = tree["child_sum"][0].cpu().numpy(), tree["child_count"][0].cpu().numpy()
    assert np.array_equal(got_sum.view(np.int64), want.view(np.int64)) and np.array_equal(got_cnt, (t[..., 0].sum(axis=2) > 0).astype(np.int32))
    assert (got_cnt == 1).any()
    s.close()
    env.close()


CAPTURE_W = 5


def _capture_env():
    """5x5, two players, the playouts on the scripted rule.  Seat 0's general on (0, 0) holds 30 armies, next to a stack of 10 of
    seat 1 on (1, 0) that mountains on (2, 0) and (1, 1) box in; seat 0 has 50 armies on (2, 4), whose only open way is right
    ((1, 4) and (2, 3) are mountains), two steps from seat 1's general (army 20) on (4, 4).  Moving the general's army down
    leaves one army on the general and the stack beside it takes it on the next turn; (2, 4) right, then (3, 4) right, wins -
    on the second move, which a playout of two turns from the root does not reach (the rule itself captures a turn later)."""
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    W = CAPTURE_W
    env = GeneralsSelfPlayVecEnv(2, board_width=W, board_height=W, max_players=2, device_outputs=True, board_pool=4)
    env.reset()
    tiles = [dict(x=0, y=0, owner=0, army=30, type=1), dict(x=4, y=4, owner=1, army=20, type=1), dict(x=2, y=4, owner=0, army=50),
             dict(x=1, y=0, owner=1, army=10)] + [dict(x=x, y=y, owner=-1, army=0, type=3) for x, y in ((2, 0), (1, 1), (1, 4), (2, 3))]
    army, owner, typ = O.planes_from_tiles(W, W, tiles)
    env.engine.reset(np.stack([army] * 2), np.stack([owner] * 2), np.stack([typ] * 2))
    return env


def test_the_tree_finds_a_capture_two_moves_deep():
    import torch
    import generalsreinforcementlearning_amd as g
    W = CAPTURE_W
    env = _capture_env()
    st = env.engine.game_state()
    mask = _gym_mask(st, [0, 0, 1, 1], [0, 1, 0, 1], W, W, True)
    first, second, losing = (4 * W + 2) * 5 + 1, (4 * W + 3) * 5 + 1, 0 * 5 + 2
    assert mask[0, first] and mask[0, losing] and mask[0].sum() == 5         # the general: right, down, half; the stack: right, half
    s = g.TreeSearch(env, candidates=8, simulations=48, depth=2, replicas=1, rollout="bot")
    assert s.schedule == [(8, 2), (4, 4), (2, 8)]
    actions, info = s.act(torch.from_numpy(mask).cuda(), seed=4)
    cand, count, total = (info[k].cpu().numpy() for k in ("candidates", "count", "sum"))
    tree = {k: v.cpu().numpy() for k, v in info["tree"].items()}
    for r in (0, 2):                                                          # seat 0's rows
        assert int(actions[r]) == first, (r, int(actions[r]), cand[r].tolist(), count[r].tolist(), total[r].tolist())
        k = int(np.flatnonzero(cand[r] == first)[0])
        # it survived every round: one visit a wave, less the few whose expansion was refused (a half move the mask shows
        # and the decode does not accept becomes a dead edge and adds nothing)
        assert 12 <= count[r, k] <= 2 + 4 + 8
        child = tree["child_node"][0, r, k]
        assert child > 0 and tree["child_count"][child, r].sum() == count[r, k] - 1      # every later visit went below it
        # The root's own playouts are two turns deep and none of them ends the game in the seat's favour (the rule takes the
        # general a turn after it stands beside it): the win is seen only from the nodes below this one - by the capturing
        # move itself, or by a general's move after which the rule captures - and it is their values that carried the slot.
        assert tree["node_status"][child, r] == 1 and tree["node_value"][child, r] < 0.5
        kids = tree["child_node"][child, r]
        kids = kids[kids > 0]
        assert len(kids) >= 2 and (tree["node_value"][kids, r] == 1.0).any()
        c2 = int(np.flatnonzero(tree["child_action"][child, r] == second)[0])    # the capturing move is one of its slots
        won = tree["child_node"][child, r, c2]
        if won > 0:                                                           # where the walk tried it: a terminal, won node
            assert tree["node_status"][won, r] == 3 and tree["node_value"][won, r] == 1.0
        print("capture row", r, "root counts", count[r].tolist(), "root sums", total[r].tolist(), "below", tree["child_count"][child, r].tolist(),
              tree["child_sum"][child, r].tolist(), "second edge", int(won))
        lose = int(np.flatnonzero(cand[r] == losing)[0])
        assert count[r, lose] >= 2 and total[r, lose] / count[r, lose] < -0.5   # the general was lost below this slot
        assert count[r, lose] < count[r, k]
    s.close()
    env.close()


def test_an_arena_entrant_plays_legal_actions():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    env = GeneralsSelfPlayVecEnv(8, board_width=8, board_height=8, max_players=2, device_outputs=True, board_pool=16)

    def net(obs, mask):                                                       # a prior and a value from the observation
        n = obs.shape[0]
        return torch.zeros((n, mask.shape[-1]), device=obs.device), obs.reshape(n, -1)[:, :8].sum(dim=1).clamp(-1, 1)

    search = g.TreeSearch(env, candidates=4, simulations=8, depth=3, prior_fn=net, value_weight=0.25)
    policy = g.playout_policy(search, seed=1)
    arena = g.Arena(env, [policy, g.random_policy(seed=2)])
    invalid = torch.zeros((8, 2), dtype=torch.int32, device="cuda")
    for _ in range(6):
        out = arena.step()
        invalid += out[4]["invalid"].to(torch.int32)
    assert int(invalid.sum()) == 0 and policy._calls == 6
    search.close()
    env.close()
