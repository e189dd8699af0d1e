"""CPU-side checks of the V-trace targets: the numpy restatement (tests/_vtrace_reference.py) against the direct sum of the
paper's definition and against the GAE restatement it reduces to on-policy, the argument checks of gvec_traj_vtrace, which
answer before any device is touched, and its exports.  No call in this file passes every check: one that did would launch
a kernel on the fake pointers below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gae_reference as R
import _vtrace_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0, 40, 7, 0.99, 0.95), (1, 64, 5, 0.9, 0.5), (2, 17, 9, 1.0, 1.0), (3, 33, 4, 0.97, 0.0), (4, 128, 6, 0.99, 0.95)]


def _rollout(seed, T, N):
    rng = np.random.default_rng(seed)
    reward, value, flags = R.random_rollout(rng, T, N, p_cut=0.1, p_invalid=0.1)
    lt, lb = V.random_logps(rng, T, N)
    valid, cut = (flags & R.VALID) != 0, (flags & R.CUT) != 0
    assert valid.any() and (~valid).any() and cut.any()
    if T > 8:
        assert (cut[:-1] & valid[1:]).any()              # a CUT row followed by a valid one: the case `nvs` is cut for
    return reward, value, flags, lt, lb


# ---- the restatement ----
@pytest.mark.parametrize("seed,T,N,gamma,lam", CASES)
@pytest.mark.parametrize("bars", [(1.0, 1.0), (2.0, 0.7), (float("inf"), float("inf"))], ids=["1_1", "2_0.7", "inf"])
def test_restatement_equals_the_direct_sum(seed, T, N, gamma, lam, bars):
    reward, value, flags, lt, lb = _rollout(seed, T, N)
    vs, pg, rho, _ = V.vtrace(reward, value, flags, lt, lb, gamma, lam, *bars)
    want, scale = V.direct(reward, value, flags, lt, lb, gamma, lam, *bars)
    err = np.abs(vs - want)
    print(f"T{T} N{N} bars {bars}: max |vs - direct| {err.max():.3g}")
    assert np.all(err <= T * 2.0 ** -52 * np.maximum(scale, 1e-300))
    valid = (flags & R.VALID) != 0
    v = value.astype(np.float64)[:-1]
    assert np.all(pg[~valid] == 0.0) and np.all(rho[~valid] == 0.0) and np.all(vs[~valid] == v[~valid])


@pytest.mark.parametrize("seed,T,N,gamma,lam", CASES)
@pytest.mark.parametrize("bars", [(1.0, 1.0), (1.0, 2.0), (float("inf"), 1.0)], ids=["1_1", "1_2", "inf_1"])
def test_on_policy_vs_is_the_gae_return_exactly(seed, T, N, gamma, lam, bars):
    reward, value, flags, _, lb = _rollout(seed, T, N)
    vs, _, rho, _ = V.vtrace(reward, value, flags, lb, lb, gamma, lam, *bars)
    _, ret = R.gae(reward, value, flags, gamma, lam)
    assert np.array_equal(vs, ret)
    assert set(np.unique(rho)) == {0.0, 1.0}


@pytest.mark.parametrize("seed,T,N,gamma,lam", CASES)
def test_on_policy_pg_at_lambda_one_is_the_gae_advantage(seed, T, N, gamma, lam):
    """pg = (r + gamma (V' + acc')) - V and adv = ((r + gamma V') - V) + gamma acc' are the same sum in another order.
    Scale: M_n bounds every magnitude either form passes through in a row, and an error carried from row t + 1 is
    multiplied by gamma <= 1, so the T * 2^-52 * scale rule of test_rollout_reference.py applies with scale = M_n."""
    reward, value, flags, _, lb = _rollout(seed, T, N)
    _, pg, _, M = V.vtrace(reward, value, flags, lb, lb, gamma, 1.0, 1.0, 1.0)
    adv, _ = R.gae(reward, value, flags, gamma, 1.0)
    err = np.abs(pg - adv)
    print(f"T{T} N{N}: max |pg - adv| {err.max():.3g}")
    assert np.all(err <= T * 2.0 ** -52 * np.maximum(M, 1e-300)[None, :])


def test_the_cut_clause_of_nvs_is_what_makes_the_identities_hold():
    """Without `CUT ? V[t+1]`, pg of a CUT row that a valid row follows would bootstrap from that row's vs."""
    reward, value, flags, _, lb = _rollout(0, 40, 7)
    _, pg, _, _ = V.vtrace(reward, value, flags, lb, lb, 0.99, 1.0, 1.0, 1.0)
    adv, ret = R.gae(reward, value, flags, 0.99, 1.0)
    v = value.astype(np.float64)
    cut = ((flags & R.CUT) != 0) & ((flags & R.TERMINAL) == 0)
    follows = np.zeros_like(cut)
    follows[:-1] = (flags[1:] & R.VALID) != 0
    rows = cut & follows
    assert rows.any()
    wrong = (reward[:-1] + 0.99 * ret[1:]) - v[:-2]             # bootstrapping from vs of row t + 1 instead
    assert np.abs(wrong[rows[:-1]] - adv[:-1][rows[:-1]]).max() > 1e-3
    assert np.abs(pg[rows] - adv[rows]).max() < 1e-12


def test_clipped_rows_give_exactly_rho_bar():
    reward, value, flags, lt, lb = _rollout(7, 64, 16)
    valid = (flags & R.VALID) != 0
    for rho_bar in (1.0, 0.75, 1.5):
        _, _, rho, _ = V.vtrace(reward, value, flags, lt, lb, 0.99, 0.95, rho_bar, 1.0)
        w = np.exp(lt.astype(np.float64) - lb.astype(np.float64))
        clipped = valid & (w >= rho_bar)
        assert clipped.any() and (valid & ~clipped).any()
        assert np.all(rho[clipped] == rho_bar) and np.all(rho[valid & ~clipped] == w[valid & ~clipped])
        assert np.all(rho.astype(np.float32)[clipped] == np.float32(rho_bar))
    _, _, rho, _ = V.vtrace(reward, value, flags, lt, lb, 0.99, 0.95, 1.0, 1.0)
    share = (rho[valid] == 1.0).mean()
    print(f"clipped share at rho_bar = 1: {share:.3f}")
    assert 0.35 < share < 0.55


# ---- the ABI without a GPU ----
@pytest.fixture(scope="module")
def L():
    from generalsreinforcementlearning_amd.csrc import build as B
    B.build(verbose=False)
    import generalsreinforcementlearning_amd as g
    return g.load()


P, ODD = 256, 264                                             # a fake aligned "device pointer", and one that is not 16-byte aligned
GOOD = dict(T=8, N=4, gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0)
INF, NAN = float("inf"), float("nan")


def _args(**over):
    from generalsreinforcementlearning_amd._lib import TrajVtraceArgs
    a = TrajVtraceArgs()
    for name, typ in TrajVtraceArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, P)
    for k, v in {**GOOD, **over}.items():
        setattr(a, k, v)
    return a


def _refused(L, a, text):
    L.gvec_traj_record(0, None, None)                         # leaves another entry point's message behind
    rc = L.gvec_traj_vtrace(0, None, C.byref(a) if a is not None else None)
    msg = L.gvec_last_error()
    assert rc == -1, rc                                       # GVEC_E_INVALID
    assert msg and ("gvec_traj_vtrace: " + text).encode() in msg, msg


def test_vtrace_refuses_bad_arguments_without_a_gpu(L):
    from generalsreinforcementlearning_amd._lib import TrajVtraceArgs
    null = "args or a required pointer is NULL"
    aligned = "scratch must be 16-byte aligned"
    _refused(L, None, null)
    for over in (dict(T=0), dict(T=-1), dict(N=0), dict(N=-5)):
        _refused(L, _args(**over), "T %d, N %d: both must be >= 1" % (over.get("T", 8), over.get("N", 4)))
    for over in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=NAN), dict(lam=-0.1), dict(lam=1.01), dict(lam=NAN)):
        _refused(L, _args(**over), "gamma")
    for over in (dict(rho_bar=0.0), dict(rho_bar=-1.0), dict(rho_bar=NAN), dict(rho_bar=-INF), dict(c_bar=0.0), dict(c_bar=-0.5),
                 dict(c_bar=NAN)):
        _refused(L, _args(**over), "rho_bar")
    pointers = [n for n, typ in TrajVtraceArgs._fields_ if typ is C.c_void_p]
    assert len(pointers) == 10
    for name in pointers:
        if name == "rho_out":                                 # optional: goes on to the next check
            _refused(L, _args(rho_out=None, scratch=ODD), aligned)
        else:
            _refused(L, _args(**{name: None}), null)
    _refused(L, _args(scratch=ODD), aligned)
    # +inf means no clipping and passes: the next check answers
    _refused(L, _args(rho_bar=INF, c_bar=INF, scratch=ODD), aligned)
    # order: shape, discounts, bars, pointers, alignment
    _refused(L, _args(T=0, gamma=2.0, rho_bar=0.0, vs=None, scratch=ODD), "T 0")
    _refused(L, _args(gamma=2.0, rho_bar=0.0, vs=None, scratch=ODD), "gamma")
    _refused(L, _args(rho_bar=0.0, vs=None, scratch=ODD), "rho_bar")
    _refused(L, _args(vs=None, scratch=ODD), null)


def test_scratch_covers_four_partials_per_wavefront(L):
    for T, N in ((1, 1), (128, 8192), (2, 65), (16, 1 << 20)):
        assert L.gvec_traj_scratch_bytes(T, N) >= (N + 63) // 64 * 4 * 8


def test_vtrace_is_exported_and_documented(L):
    from generalsreinforcementlearning_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "generals_vec.h")).read()
    assert re.search(r"int32_t gvec_traj_vtrace\(int32_t device, void\* hip_stream, const gvec_traj_vtrace_args\* args\);", hdr)
    assert "gvec_traj_vtrace" in _lib.SYMBOLS and hasattr(L, "gvec_traj_vtrace")
    assert "`gvec_traj_vtrace`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert L.gvec_abi_version() == 2
    # the struct in _lib.py has the header's fields in the header's order
    body = re.search(r"typedef struct gvec_traj_vtrace_args \{(.*?)\} gvec_traj_vtrace_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r".*[\s*]", "", d.strip()) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    assert names == [{"lam": "lambda"}.get(n, n) for n, _ in _lib.TrajVtraceArgs._fields_], names
