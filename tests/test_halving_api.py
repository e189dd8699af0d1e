"""The host side of the sequential-halving search: the exports, the argument checks of gvec_search_halve and
gvec_search_improved_policy (refused before anything touches a device) and every ValueError of the Python front
(HalvingSearch), on a stand-in engine and CPU tensors.  The file runs with and without a device, so its calls of the entry
points go through tests/_api_calls.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

HALVE, POLICY = "gvec_search_halve", "gvec_search_improved_policy"
P = 4096                                 # stands for a device pointer: never dereferenced by a call that is refused


class _HalveArgs(lib.SearchHalveArgs):
    rows = property(lambda self: self.n)         # what _api_calls.passes_checks asks for


class _PolicyArgs(lib.SearchPolicyArgs):
    rows = property(lambda self: self.n)


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


def _halve(**kw):
    a = dict(n=3, m=16, k=8, replicas=2, k_next=4, reserved=0, terms=P, slot=P, candidates0=P, prior_key=P, win=1.0, loss=-1.0,
             land=0.5, army=0.5, q_lo=-1.0, q_inv_range=0.5, c_visit=50.0, c_scale=1.0, sum=P, count=P, next_slot=P, next_candidates=P)
    a.update(kw)
    return _HalveArgs(**a)


def _policy(**kw):
    a = dict(n=3, num_actions=125, m=16, reserved=0, logits=P, mask=P, candidates0=P, sum=P, count=P, value=P, q_lo=-1.0,
             q_inv_range=0.5, c_visit=50.0, c_scale=1.0, target=P, v_mix=P)
    a.update(kw)
    return _PolicyArgs(**a)


def test_the_library_and_the_package_export_the_feature(L):
    import generalsreinforcementlearning_amd as g
    for fn in (HALVE, POLICY):
        assert hasattr(L, fn) and fn in lib.SYMBOLS
    assert C.sizeof(lib.SearchHalveArgs) == 6 * 4 + 4 * 8 + 8 * 8 + 4 * 8        # the header's gvec_search_halve_args
    assert C.sizeof(lib.SearchPolicyArgs) == 4 * 4 + 6 * 8 + 4 * 8 + 2 * 8       # ... and gvec_search_policy_args
    assert lib.SEARCH_MAX_SLOTS == 64
    assert callable(g.HalvingSearch) and callable(g.halving_schedule) and {"HalvingSearch", "halving_schedule"} <= set(g.__all__)
    assert L.gvec_abi_version() == 2


def test_halve_refuses_bad_arguments_without_a_device(L):
    rejected(L, HALVE, None, "is NULL")
    for name in ("terms", "candidates0", "prior_key", "sum", "count", "next_slot", "next_candidates"):
        rejected(L, HALVE, _halve(**{name: None}), "is NULL")
    rejected(L, HALVE, _halve(n=-1), "n -1")
    for m in (0, 65, -3):
        rejected(L, HALVE, _halve(m=m, k=1, k_next=1), f"m {m} outside")
    rejected(L, HALVE, _halve(k=17), "k 17 outside")
    rejected(L, HALVE, _halve(k=0, k_next=0), "k 0 outside")
    rejected(L, HALVE, _halve(k_next=9), "k_next 9 outside")
    rejected(L, HALVE, _halve(k_next=0), "k_next 0 outside")
    rejected(L, HALVE, _halve(replicas=0), "replicas 0")
    rejected(L, HALVE, _halve(reserved=1), "reserved")
    rejected(L, HALVE, _halve(slot=None), "slot is NULL")                        # the identity needs k == m
    passes_checks(L, HALVE, _halve(n=0))
    passes_checks(L, HALVE, _halve(n=0, slot=None, k=16, k_next=16))
    passes_checks(L, HALVE, _halve(n=0, m=64, k=64, k_next=1, slot=None))
    passes_checks(L, HALVE, _halve())                                            # with a device present: not called
    passes_checks(L, HALVE, _halve(slot=None, m=1, k=1, k_next=1))


def test_improved_policy_refuses_bad_arguments_without_a_device(L):
    rejected(L, POLICY, None, "is NULL")
    for name in ("mask", "candidates0", "sum", "count", "target", "v_mix"):
        rejected(L, POLICY, _policy(**{name: None}), "is NULL")
    rejected(L, POLICY, _policy(n=-2), "n -2")
    for m in (0, 65):
        rejected(L, POLICY, _policy(m=m), f"m {m} outside")
    for A in (0, -5, 5 * 32 * 32 + 1):
        rejected(L, POLICY, _policy(num_actions=A), f"num_actions {A} outside")
    rejected(L, POLICY, _policy(reserved=7), "reserved")
    passes_checks(L, POLICY, _policy(n=0))
    passes_checks(L, POLICY, _policy(n=0, logits=None, value=None, num_actions=5 * 32 * 32, m=64))
    passes_checks(L, POLICY, _policy(logits=None, value=None))


# ---- the Python front -------------------------------------------------------------------------------------------------------
def _engine(W=3, H=2, P_=2):
    """what HalvingSearch reads of an engine; nothing here calls the library"""
    return types.SimpleNamespace(max_w=W, max_h=H, max_p=P_, B=4, device=0)


def test_the_constructor_refuses_bad_arguments():
    from generalsreinforcementlearning_amd import HalvingSearch, PlayoutScore
    for bad in (dict(candidates=0), dict(candidates=65), dict(candidates=2.0), dict(candidates=True), dict(budget=0), dict(budget="64"),
                dict(depth=0), dict(depth=None), dict(c_visit=-1.0), dict(c_visit=float("nan")), dict(c_scale=float("inf")),
                dict(c_scale="1"), dict(score=lambda t: t), dict(score=PlayoutScore(win=0.0, loss=0.0, land=0.0, army=0.0)),
                dict(rollout="minimax"), dict(bot_players=[0]), dict(bot_random_permille=5),
                dict(rollout="bot", bot_random_permille=1001), dict(rollout="bot", bot_players=[2])):
        with pytest.raises(ValueError):
            HalvingSearch(_engine(), **bad)
    s = HalvingSearch(_engine(), candidates=16, budget=64, depth=8)
    assert s.schedule == [(16, 1), (8, 2), (4, 4), (2, 8)] and s.playouts_per_row == 64 and s.num_actions == 30
    assert (s.q_lo, s.q_inv_range, s.c_visit, s.c_scale) == (-1.0, 0.5, 50.0, 1.0)
    w = HalvingSearch(_engine(), score=PlayoutScore(win=2.0, loss=-0.25, land=1.0, army=1.0))
    assert w.q_lo == -1.0 and w.q_inv_range == 1.0 / 3.0
    b = HalvingSearch(_engine(P_=4), candidates=4, budget=8, rollout="bot", bot_players=[1, 3], bot_random_permille=100)
    assert (b.rollout, b.bot_players, b.bot_random_permille) == ("bot", 0b1010, 100)
    assert [(r.K, r.R, r.D, r.rollout, r.bot_players) for r in b._rounds] == [(4, 1, 8, "bot", 0b1010), (2, 2, 8, "bot", 0b1010)]
    assert HalvingSearch.round_seed(5, 0) != HalvingSearch.round_seed(5, 1) and 0 <= HalvingSearch.round_seed(2 ** 64 - 1, 3) < 2 ** 64


def test_the_methods_refuse_bad_arguments_before_any_library_call():
    from generalsreinforcementlearning_amd import HalvingSearch
    s = HalvingSearch(_engine(), candidates=4, budget=8, depth=2)
    A = s.num_actions
    for mask in (torch.zeros(2, A + 1, dtype=torch.bool), torch.zeros(2, A, dtype=torch.float32), torch.zeros(A, dtype=torch.bool),
                 np.zeros((2, A), bool)):
        with pytest.raises(ValueError):
            s.propose(mask)
    with pytest.raises(ValueError):
        s.propose(torch.zeros(2, A, dtype=torch.bool), torch.zeros(2, A, dtype=torch.int64))
    with pytest.raises(ValueError):
        s.propose(torch.zeros(2, A, dtype=torch.bool), torch.zeros(3, A))
    # search, act and policy_target: CPU tensors are on the wrong device, and are refused before the engine (a stand-in) is touched
    cand, prior, players = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="is on cpu"):
        s.search(None, players, cand, prior)
    with pytest.raises(ValueError, match="is on cpu"):
        s.act(torch.zeros(2, A, dtype=torch.bool))
    for bad in (lambda: s.search(None, players, cand.to(torch.int32), prior), lambda: s.search(None, players, "candidates", prior),
                lambda: s.search(None, players, cand[:, :3], prior)):
        with pytest.raises(ValueError):
            bad()
    info = dict(candidates=cand, sum=prior, count=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="is on cpu"):
        s.policy_target(torch.zeros(2, A), torch.zeros(2, A, dtype=torch.bool), info)
    for bad in (lambda: s.policy_target(None, torch.zeros(2, A), info), lambda: s.policy_target(None, "mask", info),
                lambda: s.policy_target(None, np.zeros((2, A), bool), info)):
        with pytest.raises(ValueError):
            bad()
