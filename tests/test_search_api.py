"""The host side of the playout search (generalsreinforcementlearning_amd/search.py): the export of gvec_search_playouts, the
score, the reductions, the proposal and the argument checks of the Python front, on CPU tensors.  The file runs with and
without a device, so its one call of the entry point goes through tests/_api_calls.py."""
import types

import numpy as np
import pytest
import torch

from _api_calls import rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

FN = "gvec_search_playouts"


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


def test_the_library_exports_the_entry_point(L):
    assert hasattr(L, FN) and FN in lib.SYMBOLS
    assert (lib.SEARCH_TERMS, lib.SEARCH_PASS, lib.SEARCH_NONE) == (8, -1, -2)
    import ctypes as C
    assert C.sizeof(lib.SearchArgs) == 16 + 3 * 8 + 8 + 8                    # the header's gvec_search_args


def test_null_handle_and_null_args_are_refused(L):
    """_api_calls hands every entry point (0, None, args): for this one, whose parameters are (h, args), that is the NULL
    handle with NULL args, whatever `args` is - the one refusal this module can ask for.  The checks of the fields are in
    tests/test_search_args.py."""
    rejected(L, FN, None, "is NULL")


def test_the_package_exports_the_front():
    import generalsreinforcementlearning_amd as g
    assert callable(g.PlayoutSearch) and callable(g.PlayoutScore) and callable(g.playout_policy)
    assert {"PlayoutSearch", "PlayoutScore", "playout_policy"} <= set(g.__all__)
    assert callable(g.VecEngine.search_playouts_device)


# ---- the reductions on hand-written terms, against numpy float64 ------------------------------------------------------------
def _engine(W=3, H=2):
    """what PlayoutSearch reads of an engine; nothing here calls the library"""
    return types.SimpleNamespace(max_w=W, max_h=H, max_p=2, B=4, device=0)


#        valid turns alive won land army land_o army_o
TERMS = np.array([
    [[[1, 8, 1, 0, 10, 50, 5, 25], [1, 8, 1, 0, 3, 7, 9, 100]],             # row 0, candidate 0: two ordinary replicas
     [[1, 3, 1, 1, 25, 90, 0, 0], [1, 8, 1, 0, 12, 40, 12, 40]],            # candidate 1: one replica won (others hold nothing)
     [[1, 2, 0, 0, 0, 0, 25, 130], [1, 5, 0, 0, 0, 0, 20, 99]]],            # candidate 2: the seat died in both
    [[[1, 8, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]],                  # row 1, candidate 0: zero denominators; one replica invalid
     [[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]],                  # candidate 1: invalid
     [[0, 0, 0, 0, 0, 0, 0, 0], [1, 8, 1, 0, 7, 0, 7, 0]]],                 # candidate 2: army denominators zero, one replica invalid
    [[[0, 0, 0, 0, 0, 0, 0, 0]] * 2] * 3,                                   # row 2: no valid candidate at all
], dtype=np.int32)
WEIGHTS = [dict(), dict(win=2.0, loss=-3.0, land=0.25, army=1.5)]


def _np_score(t, win=1.0, loss=-1.0, land=0.5, army=0.5):
    t = t.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rl = np.where(t[..., 4] + t[..., 6] != 0, t[..., 4] / (t[..., 4] + t[..., 6]), 0.5)
        ra = np.where(t[..., 5] + t[..., 7] != 0, t[..., 5] / (t[..., 5] + t[..., 7]), 0.5)
    s = land * rl + army * ra - (land + army) / 2
    s = np.where(t[..., 2] == 0, loss, s)
    return np.where(t[..., 3] != 0, win, s)


def _np_scores(t, **kw):
    ok = t[..., 0] != 0
    s = np.where(ok, _np_score(t, **kw), 0.0)
    cnt = ok.sum(-1)
    return (s.sum(-1) / np.maximum(cnt, 1)).astype(np.float32), cnt > 0


def _close(got, want, ctx=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (ctx, got, want)


@pytest.mark.parametrize("kw", WEIGHTS, ids=["default", "weighted"])
def test_playout_score_equals_the_numpy_restatement(kw):
    from generalsreinforcementlearning_amd import PlayoutScore
    got = PlayoutScore(**kw)(torch.from_numpy(TERMS))
    assert got.dtype == torch.float64 and tuple(got.shape) == TERMS.shape[:-1]
    _close(got.numpy(), _np_score(TERMS, **kw))
    d = {**dict(win=1.0, loss=-1.0, land=0.5, army=0.5), **kw}
    assert got[0, 1, 0] == d["win"] and got[0, 2, 0] == d["loss"] and got[1, 0, 0] == 0.0     # won, dead, 0 / 0 twice: the middle
    with pytest.raises(ValueError):
        PlayoutScore()(torch.zeros(3, 7, dtype=torch.int32))
    with pytest.raises(ValueError):
        PlayoutScore()(torch.zeros(3, 8, dtype=torch.int64))


@pytest.mark.parametrize("kw", WEIGHTS, ids=["default", "weighted"])
def test_scores_equal_the_numpy_restatement(kw):
    from generalsreinforcementlearning_amd import PlayoutScore, PlayoutSearch
    s = PlayoutSearch(_engine(), candidates=3, replicas=2, depth=8, score=PlayoutScore(**kw))
    q, valid = s.scores(torch.from_numpy(TERMS))
    wq, wv = _np_scores(TERMS, **kw)
    assert q.dtype == torch.float32 and valid.dtype == torch.bool
    assert np.array_equal(valid.numpy(), wv) and wv.tolist() == [[True] * 3, [True, False, True], [False] * 3]
    _close(q.numpy(), wq)
    with pytest.raises(ValueError):
        s.scores(torch.from_numpy(TERMS[0]))


@pytest.mark.parametrize("temperature", [1.0, 0.25, 3.0])
def test_policy_target_equals_the_numpy_restatement(temperature):
    from generalsreinforcementlearning_amd import PlayoutSearch
    s = PlayoutSearch(_engine(), candidates=3, replicas=2, depth=8)
    A = s.num_actions
    assert A == 30
    q, valid = s.scores(torch.from_numpy(TERMS))
    cand = torch.tensor([[7, 0, 29], [3, lib.SEARCH_NONE, 11], [lib.SEARCH_NONE] * 3], dtype=torch.int64)
    got = s.policy_target(cand, q, valid, temperature=temperature)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, A)
    want = np.zeros((3, A))
    qn, vn = q.numpy().astype(np.float64), valid.numpy()
    for r in range(3):
        if vn[r].any():
            z = qn[r][vn[r]] / temperature
            e = np.exp(z - z.max())
            want[r, cand[r].numpy()[vn[r]]] = e / e.sum()
    _close(got.numpy(), want.astype(np.float32))
    sums = got.double().sum(1).numpy()
    assert abs(sums[0] - 1) < 1e-6 and abs(sums[1] - 1) < 1e-6 and sums[2] == 0.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            s.policy_target(cand, q, valid, temperature=bad)
    with pytest.raises(ValueError):
        s.policy_target(cand.to(torch.int32), q, valid)
    with pytest.raises(ValueError):
        s.policy_target(cand, q[:, :2], valid)
    with pytest.raises(ValueError):
        s.policy_target(cand, q, valid.to(torch.uint8))


def test_propose_takes_the_top_legal_actions_and_pads():
    from generalsreinforcementlearning_amd import PlayoutSearch
    s = PlayoutSearch(_engine(), candidates=4, replicas=1, depth=1)
    A = s.num_actions
    mask = torch.zeros(4, A, dtype=torch.bool)
    mask[0, [2, 5, 9, 14, 20, 21]] = True
    mask[1, [3, 8]] = True                                                   # fewer legal actions than K
    mask[3, :] = True
    logits = torch.arange(A, dtype=torch.float32).repeat(4, 1)
    logits[0, 9] = 100.0
    c = s.propose(mask, logits)
    assert c.dtype == torch.int64 and tuple(c.shape) == (4, 4) and c.is_contiguous()
    assert c[0].tolist() == [9, 21, 20, 14] and c[1].tolist() == [8, 3, lib.SEARCH_NONE, lib.SEARCH_NONE]
    assert c[2].tolist() == [lib.SEARCH_NONE] * 4 and c[3].tolist() == [29, 28, 27, 26]
    # no prior: distinct legal actions, the same for the same seed, others for another, uint8 masks alike
    u = s.propose(mask, None, seed=5)
    assert torch.equal(u, s.propose(mask.to(torch.uint8), None, seed=5)) and not torch.equal(u, s.propose(mask, None, seed=6))
    assert sorted(u[1].tolist()) == [lib.SEARCH_NONE, lib.SEARCH_NONE, 3, 8] and u[2].tolist() == [lib.SEARCH_NONE] * 4
    assert set(u[0].tolist()) <= {2, 5, 9, 14, 20, 21} and len(set(u[0].tolist())) == 4 and len(set(u[3].tolist())) == 4
    # more candidates than actions: the tail is padding
    wide = PlayoutSearch(_engine(1, 1), candidates=7, replicas=1, depth=1)
    assert wide.propose(torch.ones(1, 5, dtype=torch.bool), torch.zeros(1, 5))[0, 5:].tolist() == [lib.SEARCH_NONE] * 2


def test_bad_arguments_raise_before_any_library_call():
    from generalsreinforcementlearning_amd import PlayoutSearch
    for bad in (dict(candidates=0), dict(replicas=0), dict(depth=0), dict(candidates=2.5), dict(depth=True)):
        with pytest.raises(ValueError):
            PlayoutSearch(_engine(), **bad)
    s = PlayoutSearch(_engine(), candidates=3, replicas=2, depth=4)
    A = s.num_actions
    for mask in (torch.zeros(2, A + 1, dtype=torch.bool), torch.zeros(2, A, dtype=torch.float32), torch.zeros(A, dtype=torch.bool),
                 np.zeros((2, A), bool)):
        with pytest.raises(ValueError):
            s.propose(mask)
    with pytest.raises(ValueError):
        s.propose(torch.zeros(2, A, dtype=torch.bool), torch.zeros(2, A, dtype=torch.int64))
    with pytest.raises(ValueError):
        s.propose(torch.zeros(2, A, dtype=torch.bool), torch.zeros(3, A))
    # evaluate and act: CPU tensors are on the wrong device, and are refused before the engine (a stand-in here) is touched
    cand = torch.zeros(2, 3, dtype=torch.int64)
    players = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="is on cpu"):
        s.evaluate(None, players, cand)
    with pytest.raises(ValueError, match="is on cpu"):
        s.act(torch.zeros(2, A, dtype=torch.bool))
    with pytest.raises(ValueError):
        s.evaluate(None, players, cand.to(torch.int32))
    with pytest.raises(ValueError):
        s.evaluate(None, players, "candidates")
