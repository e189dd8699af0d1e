"""V-trace targets on the GPU: gvec_traj_vtrace against its numpy restatement (tests/_vtrace_reference.py),
SelfPlayRolloutBuffer.finish_vtrace / evaluate_rollout on a real env, and the example with a lagging actor.

Tolerance of an element of vs or pg:  |out - f32(ref)| <= spacing32(f32(ref)) + T * 2^-48 * M_n.  The first term is the one
rounding to float32.  The second bounds fewer than 16 float64 operations per row (exp included) at 2^-53 relative each, on
magnitudes M_n bounds, carried over at most T rows - which holds while gamma * lambda * c <= 1, so these cases use c_bar <= 1;
the unclipped case keeps |log ratio| <= 0.25 over T <= 16 rows and multiplies the term by e^4, the largest product of T
such factors."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import _gae_reference as R
import _vtrace_reference as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, LAM = 0.99, 0.95
INF = float("inf")


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar, with_rho=True):
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import TrajVtraceArgs, check
    T, N = reward.shape
    L = g.load()
    d = [_dev(x) for x in (reward, value, flags, lb, lt)]
    vs, pg, rho = (torch.full((T, N), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3))
    stats = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(T, N)), dtype=torch.uint8, device="cuda")
    a = TrajVtraceArgs(T=T, N=N, gamma=gamma, lam=lam, rho_bar=rho_bar, c_bar=c_bar, reward=d[0].data_ptr(), value=d[1].data_ptr(),
                       flags=d[2].data_ptr(), logp_behaviour=d[3].data_ptr(), logp_target=d[4].data_ptr(), vs=vs.data_ptr(),
                       pg=pg.data_ptr(), rho_out=rho.data_ptr() if with_rho else None, stats=stats.data_ptr(), scratch=scratch.data_ptr())
    check(L.gvec_traj_vtrace(0, torch.cuda.current_stream().cuda_stream, C.byref(a)), "gvec_traj_vtrace")
    torch.cuda.synchronize()
    return vs.cpu().numpy(), pg.cpu().numpy(), rho.cpu().numpy(), stats.cpu().numpy()


def _assert_close(name, got, want64, slack, ctx):
    """|got - f32(want)| <= spacing32(f32(want)) + slack, elementwise; prints the largest ulp distance first."""
    want = want64.astype(np.float32)
    ulp = R.ulp_diff(got, want)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = np.spacing(np.abs(want)).astype(np.float64) + slack
    print(f"{ctx}: {name} max ulp {ulp.max()}, max err / bound {(err / bound).max():.3g}")
    assert np.all(err <= bound), (ctx, name)


def _assert_vtrace(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar, ctx, growth=1.0):
    T, N = reward.shape
    vs, pg, rho, st = _run(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar)
    want_vs, want_pg, want_rho, M = V.vtrace(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar)
    slack = (growth * T * 2.0 ** -48 * M)[None, :]
    _assert_close("vs", vs, want_vs, slack, ctx)
    _assert_close("pg", pg, want_pg, slack, ctx)
    du = R.ulp_diff(rho, want_rho.astype(np.float32))
    print(f"{ctx}: rho max ulp {du.max()}, clipped share {(want_rho == rho_bar).mean():.3f}")
    assert du.max() <= 1, ctx
    assert np.all(rho[want_rho == rho_bar] == np.float32(rho_bar)), ctx
    valid = (flags & R.VALID) != 0
    assert not rho[~valid].any() and not pg[~valid].any() and np.array_equal(vs[~valid], value[:-1][~valid]), ctx
    # statistics: of the values as stored
    want = V.stats(pg, rho, flags)
    x = pg.astype(np.float64)[valid]
    print(f"{ctx}: stats {st} want {want}")
    assert st[0] == want[0], ctx
    for k, s_abs in ((1, np.abs(x).sum()), (2, (x * x).sum()), (3, rho.astype(np.float64)[valid].sum())):
        assert abs(st[k] - want[k]) <= T * N * 2.0 ** -53 * s_abs, (ctx, k)
    # the same input gives the same bits, and rho_out = NULL changes nothing else
    again = _run(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((vs, pg, rho, st), again)), ctx
    vs3, pg3, rho3, st3 = _run(reward, value, flags, lt, lb, gamma, lam, rho_bar, c_bar, with_rho=False)
    assert vs3.tobytes() == vs.tobytes() and pg3.tobytes() == pg.tobytes() and st3.tobytes() == st.tobytes(), ctx
    assert np.isnan(rho3).all(), ctx                                # never written
    return vs, pg, rho, st


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------
# N = 16,448: 257 per-wavefront partials, so a thread of the statistics' second stage (stride 256) adds two
VTRACE_CASES = [(T, N) for T in (1, 2, 33, 128) for N in (1, 63, 64, 65, 8192)] + [(2, 16448)]


@pytest.mark.parametrize("T,N", VTRACE_CASES, ids=[f"{N}-{T}" for T, N in VTRACE_CASES])
def test_vtrace_against_the_restatement(T, N):
    rng = np.random.default_rng(1000 * T + N)
    reward, value, flags = R.random_rollout(rng, T, N)
    lt, lb = V.random_logps(rng, T, N)
    _assert_vtrace(reward, value, flags, lt, lb, GAMMA, LAM, 1.0, 1.0, f"T{T} N{N}")


@pytest.mark.parametrize("rho_bar,c_bar", [(1.5, 0.8), (0.5, 1.0), (INF, 1.0)], ids=["1.5_0.8", "0.5_1", "inf_1"])
def test_vtrace_other_truncation_levels(rho_bar, c_bar):
    rng = np.random.default_rng(17)
    T, N = 33, 65
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.1, p_invalid=0.1)
    lt, lb = V.random_logps(rng, T, N)
    _assert_vtrace(reward, value, flags, lt, lb, GAMMA, LAM, rho_bar, c_bar, f"rho_bar {rho_bar} c_bar {c_bar}")


@pytest.mark.parametrize("pattern", ["cut_everywhere", "no_cut", "all_invalid", "terminal_everywhere"])
def test_vtrace_flag_extremes(pattern):
    rng = np.random.default_rng(3)
    T, N = 128, 65
    reward, value, _ = R.random_rollout(rng, T, N)
    lt, lb = V.random_logps(rng, T, N)
    f = {"cut_everywhere": R.VALID | R.CUT, "no_cut": R.VALID, "all_invalid": 0, "terminal_everywhere": R.VALID | R.CUT | R.TERMINAL}[pattern]
    flags = np.full((T, N), f, np.uint8)
    vs, pg, rho, st = _assert_vtrace(reward, value, flags, lt, lb, GAMMA, LAM, 1.0, 1.0, pattern)
    if pattern == "all_invalid":
        assert not pg.any() and not rho.any() and np.array_equal(vs, value[:-1]) and not st.any()


def test_vtrace_unclipped():
    rng = np.random.default_rng(5)
    T, N = 16, 65
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.02, p_invalid=0.02)
    lb = (-3.0 * rng.random((T, N))).astype(np.float32)
    lt = (lb + rng.uniform(-0.24, 0.24, (T, N)).astype(np.float32)).astype(np.float32)
    assert np.abs(lt.astype(np.float64) - lb.astype(np.float64)).max() <= 0.25
    _assert_vtrace(reward, value, flags, lt, lb, GAMMA, LAM, INF, INF, "unclipped", growth=math.e ** 4)


def test_vtrace_on_policy_is_gae():
    """Equal log-probs, bars >= 1: vs is gvec_traj_gae's ret, byte for byte (exp(0) = 1 and a product with 1 are exact)."""
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd._lib import TrajGaeArgs, check
    rng = np.random.default_rng(8)
    T, N = 33, 65
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.1, p_invalid=0.1)
    _, lb = V.random_logps(rng, T, N)
    vs, _, rho, _ = _run(reward, value, flags, lb, lb, GAMMA, LAM, 1.0, 2.0)
    L = g.load()
    d = [_dev(x) for x in (reward, value, flags)]
    adv, ret = (torch.empty((T, N), dtype=torch.float32, device="cuda") for _ in range(2))
    stats = torch.empty(4, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(T, N)), dtype=torch.uint8, device="cuda")
    a = TrajGaeArgs(T=T, N=N, gamma=GAMMA, lam=LAM, reward=d[0].data_ptr(), value=d[1].data_ptr(), flags=d[2].data_ptr(),
                    adv=adv.data_ptr(), ret=ret.data_ptr(), stats=stats.data_ptr(), scratch=scratch.data_ptr())
    check(L.gvec_traj_gae(0, torch.cuda.current_stream().cuda_stream, C.byref(a)), "gvec_traj_gae")
    torch.cuda.synchronize()
    assert vs.tobytes() == ret.cpu().numpy().tobytes()
    assert set(np.unique(rho)) == {0.0, 1.0}


# ---- 2. the buffer on a real env -----------------------------------------------------------------------------------------
def _actions_from_mask(mask, gen):
    import torch
    B, L, K = mask.shape
    m = mask.reshape(B * L, K).float()
    m[:, 0] += (m.sum(1) == 0).float()
    return torch.multinomial(m, 1, generator=gen).reshape(B, L)


@pytest.fixture(scope="module")
def rollout():
    """One full rollout of 8 envs, 8x8, 2 learners, horizon 12 > max_turns 10: truncation and re-deal rows occur."""
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    B, L, T = 8, 2, 12
    env = GeneralsSelfPlayVecEnv(B, 8, 8, 2, max_turns=10, seed=3, board_pool=16, device_outputs=True)
    buf = g.SelfPlayRolloutBuffer(env, T, gamma=GAMMA, gae_lambda=LAM)
    buf.begin(*env.reset())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    with pytest.raises(RuntimeError):
        buf.finish_vtrace(torch.zeros(B, L, device="cuda"), torch.zeros(T, B, L, device="cuda"))
    while not buf.full:
        a = _actions_from_mask(buf.valid_actions_mask, gen)
        buf.step(a, -3.0 * torch.rand(B, L, device="cuda", generator=gen), torch.randn(B, L, device="cuda", generator=gen))
    last = torch.randn(B, L, device="cuda", generator=gen)
    torch.cuda.synchronize()
    host = dict(reward=buf.reward.cpu().numpy(), flags=buf.flags.cpu().numpy(), logp=buf.logp.cpu().numpy(), last=last.cpu().numpy().reshape(1, -1))
    flags = host["flags"]
    valid, cut, term = (flags & R.VALID) != 0, (flags & R.CUT) != 0, (flags & R.TERMINAL) != 0
    assert (cut & ~term).any() and (~valid).any() and valid.any()            # truncations and re-deal rows were met
    yield buf, last, host, gen
    env.close()


def _ulp(buf_tensor, want64, shape):
    return R.ulp_diff(buf_tensor.cpu().numpy().reshape(shape), want64.astype(np.float32)).max()


def test_buffer_on_policy_vtrace_and_gae(rollout):
    import torch
    buf, last, host, _ = rollout
    T, N = buf.horizon, buf.num_streams
    value = np.concatenate([buf.value[:T].cpu().numpy(), host["last"]]).astype(np.float32)
    want_adv, want_ret = R.gae(host["reward"], value, host["flags"], GAMMA, LAM)
    want_vs, want_pg, want_rho, _ = V.vtrace(host["reward"], value, host["flags"], host["logp"], host["logp"], GAMMA, LAM, 1.0, 1.0)
    assert np.array_equal(want_vs, want_ret)                                  # the two restatements agree exactly

    buf.finish(last)
    first = [x.clone() for x in (buf.advantages, buf.returns, buf.stats)]
    da, dr = _ulp(buf.advantages, want_adv, (T, N)), _ulp(buf.returns, want_ret, (T, N))
    print(f"finish: max ulp adv {da} ret {dr}")
    assert da <= 1 and dr <= 1
    with pytest.raises(RuntimeError):
        buf.rho
    assert "rho" not in buf.gather(torch.arange(5, device="cuda"))

    buf.finish_vtrace(last, buf.logp)
    assert buf.advantages.shape == buf.returns.shape == buf.rho.shape == (T, buf.num_envs, buf.num_learners)
    dp, dv = _ulp(buf.advantages, want_pg, (T, N)), _ulp(buf.returns, want_vs, (T, N))
    print(f"finish_vtrace: max ulp pg {dp} vs {dv}")
    assert dp <= 1 and dv <= 1
    assert np.array_equal(buf.rho.cpu().numpy().reshape(T, N), want_rho.astype(np.float32))
    assert torch.equal(buf.returns, first[1])                                 # vs is GAE's return on the device too
    st = buf.stats.cpu().numpy()
    valid = (host["flags"] & R.VALID) != 0
    assert st[0] == valid.sum() and st[3] == valid.sum()                      # every valid row has rho = 1

    # batches: rho and weight are the stores' rows
    pos = torch.randperm(T * N, device="cuda")[:100]
    batch = buf.gather(pos, normalize=False)
    p = pos.cpu().numpy()
    assert np.array_equal(batch["rho"].cpu().numpy(), buf.rho.cpu().numpy().reshape(-1)[p])
    assert np.array_equal(batch["weight"].cpu().numpy(), valid.reshape(-1)[p].astype(np.float32))
    assert np.array_equal(batch["advantages"].cpu().numpy(), buf.advantages.cpu().numpy().reshape(-1)[p])
    seen = [b["index"].cpu().numpy() for b in buf.minibatches(50, seed=1) if "rho" in b]
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(T * N))

    buf.finish(last)                                                          # GAE again: byte for byte what it was
    for got, was in zip((buf.advantages, buf.returns, buf.stats), first):
        assert got.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()
    assert "rho" not in buf.gather(pos)


def test_buffer_off_policy_with_fresh_values(rollout):
    import torch
    buf, last, host, gen = rollout
    T, N, B, L = buf.horizon, buf.num_streams, buf.num_envs, buf.num_learners
    target = buf.logp.view(T, B, L) + 0.5 * torch.randn(T, B, L, device="cuda", generator=gen)
    fresh = torch.randn(T, B, L, device="cuda", generator=gen)
    recorded = buf.value.clone()
    buf.finish(last)                                                          # value[T] = last, as every finish leaves it
    recorded[T] = last.view(-1)
    for rho_bar, c_bar in ((1.0, 1.0), (2.0, 0.5)):
        buf.finish_vtrace(last, target, value=fresh, rho_bar=rho_bar, c_bar=c_bar)      # and again: re-targeting
        assert torch.equal(buf.value, recorded)                               # the behaviour-time values are left alone
        value = np.concatenate([fresh.cpu().numpy().reshape(T, N), host["last"]]).astype(np.float32)
        lt = target.cpu().numpy().reshape(T, N)
        want_vs, want_pg, want_rho, M = V.vtrace(host["reward"], value, host["flags"], lt, host["logp"], GAMMA, LAM, rho_bar, c_bar)
        slack = (T * 2.0 ** -48 * M)[None, :]
        _assert_close("vs", buf.returns.cpu().numpy().reshape(T, N), want_vs, slack, f"buffer {rho_bar} {c_bar}")
        _assert_close("pg", buf.advantages.cpu().numpy().reshape(T, N), want_pg, slack, f"buffer {rho_bar} {c_bar}")
        assert R.ulp_diff(buf.rho.cpu().numpy().reshape(T, N), want_rho.astype(np.float32)).max() <= 1
        batch = buf.gather(torch.arange(T * N, device="cuda"), normalize=False)
        assert torch.equal(batch["value"], recorded[:T].view(-1)) and torch.equal(batch["rho"], buf.rho.view(-1))
        assert torch.equal(batch["returns"], buf.returns.view(-1))
    clipped = (want_rho == 2.0).sum()
    assert 0 < clipped < (want_rho > 0).sum()
    with pytest.raises(ValueError):
        buf.finish_vtrace(last, target[:-1])
    with pytest.raises(ValueError):
        buf.finish_vtrace(last, target, rho_bar=0.0)


def test_evaluate_rollout_chunked_equals_unchunked(rollout):
    import torch
    import generalsreinforcementlearning_amd as g
    buf, _, _, _ = rollout
    T, B, L = buf.horizon, buf.num_envs, buf.num_learners
    head = g.MaskedCategoricalHead(torch.device("cuda", 0))
    calls = []

    def fn(obs, memory):
        """elementwise in every row, so a row's outputs cannot depend on which rows share its chunk"""
        assert memory is None and obs.shape[1:] == (9, 8, 8) and not torch.is_grad_enabled()
        assert obs.data_ptr() == buf.obs_store.data_ptr() + 4 * 9 * 64 * sum(calls)      # a view of the store, in place
        calls.append(obs.shape[0])
        logits = (0.25 * obs[:, :5] + torch.sin(obs[:, 5:6])).permute(0, 2, 3, 1).reshape(obs.shape[0], -1)
        return logits, 0.5 * obs[:, 0, 0, 0] - obs[:, 1, 1, 1]

    whole = buf.evaluate_rollout(fn, head)
    assert calls == [T * B * L]
    calls.clear()
    chunked = buf.evaluate_rollout(fn, head, chunk_rows=7)
    assert calls == [7] * (T * B * L // 7) + [T * B * L % 7]
    for a, b in zip(whole, chunked):
        assert a.shape == (T, B, L) and a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    obs = buf.obs_store.view(-1, 9, 8, 8)[:T * B * L]
    calls.clear()
    with torch.no_grad():
        logits, value = fn(obs, None)
    logp, _ = head.evaluate(logits, buf.mask_store.view(-1, buf.mask_bytes)[:T * B * L].view(torch.bool), buf.action.view(-1))
    assert torch.equal(whole[0].view(-1), logp) and torch.equal(whole[1].view(-1), value)
    assert head.bad_actions == 0 and float(whole[0].min()) < 0.0
    with pytest.raises(ValueError):
        buf.evaluate_rollout(fn, head, chunk_rows=0)


# ---- 3. the example with a lagging actor ---------------------------------------------------------------------------------
def test_selfplay_ppo_example_with_vtrace_and_a_lagging_actor():
    spec = importlib.util.spec_from_file_location("train_ppo_selfplay", os.path.join(ROOT, "examples", "train_ppo_selfplay.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(["--num-envs", "64", "--board", "8", "--players", "2", "--horizon", "16", "--iterations", "4", "--batch-size", "512",
                  "--max-turns", "10", "--vtrace", "--actor-lag", "2"])
    rows = out["iterations"]
    assert len(rows) == 4
    for r in rows:
        print(r)
        assert all(math.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "clip_fraction", "mean_rho")), r
        assert 0.0 < r["mean_rho"] <= 1.0, r
        assert 0.0 < r["valid_rows"] < 1.0, r
    assert out["bad_actions"] == 0 and out["rejected"] == 0
    assert out["parameter_change"] > 0.0
    # iterations 0 and 2 refresh the actor, 1 and 3 act with a copy one iteration old: further off-policy, more rows clipped
    assert rows[1]["mean_rho"] < rows[0]["mean_rho"] and rows[3]["mean_rho"] < rows[2]["mean_rho"]
