"""The host side of the playout search with scripted-opponent playouts: the export of gvec_search_playouts_bot and the
argument checks of the Python front (PlayoutSearch(rollout=...), VecEngine.search_playouts_device), on a stand-in engine:
nothing here launches, and the file runs with and without a device.  The entry point takes (h, args, bot_players,
bot_random_permille), not the (device, stream, args) that tests/_api_calls.py hands over, so its own refusals - every field of
the struct, the mix, the seat mask, each by name - are asked for in tests/test_search_bot_args.py, all on a NULL handle."""
import ctypes as C
import types

import pytest
import torch

from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

FN = "gvec_search_playouts_bot"


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


def test_the_library_exports_the_entry_point(L):
    assert hasattr(L, FN) and FN in lib.SYMBOLS
    restype, argtypes = lib.SYMBOLS[FN]
    assert restype is C.c_int32 and len(argtypes) == 4 and argtypes[2] is C.c_uint32 and argtypes[3] is C.c_int32
    assert argtypes[:2] == lib.SYMBOLS["gvec_search_playouts"][1]            # the same handle and the same, unchanged struct
    assert C.sizeof(lib.SearchArgs) == 16 + 3 * 8 + 8 + 8


def test_the_header_declares_it():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "generals_vec.h")) as f:
        text = f.read()
    assert ("int32_t gvec_search_playouts_bot(gvec_handle* h, const gvec_search_args* args, uint32_t bot_players, "
            "int32_t bot_random_permille);") in text
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "`gvec_search_playouts_bot`" in f.read()


# ---- the Python front on a stand-in engine that records what it is asked ----------------------------------------------------
class _Engine(types.SimpleNamespace):
    def search_playouts_device(self, *a, **kw):
        self.calls.append((a, kw))


def _engine(max_p=4):
    return _Engine(max_w=3, max_h=2, max_p=max_p, B=4, device=0, calls=[])


def test_the_rollout_setting_is_checked_before_any_library_call():
    from generalsreinforcementlearning_amd import PlayoutSearch
    s = PlayoutSearch(_engine())
    assert (s.rollout, s.bot_players, s.bot_random_permille) == ("agent", 0, 0)
    s = PlayoutSearch(_engine(), rollout="bot")
    assert (s.rollout, s.bot_players, s.bot_random_permille) == ("bot", 0b1111, 0)           # None: every seat
    assert PlayoutSearch(_engine(2), rollout="bot").bot_players == 0b11
    assert PlayoutSearch(_engine(8), rollout="bot", bot_players=[1, 7], bot_random_permille=250).bot_players == 0b10000010
    assert PlayoutSearch(_engine(), rollout="bot", bot_players=0b0110).bot_players == 0b0110
    assert PlayoutSearch(_engine(), rollout="bot", bot_players=()).bot_players == 0
    for bad in (dict(rollout="agent", bot_players=0b1), dict(rollout="agent", bot_players=[]), dict(rollout="agent", bot_random_permille=5),
                dict(rollout="random"), dict(rollout=None), dict(rollout="bot", bot_players=0b10000), dict(rollout="bot", bot_players=[4]),
                dict(rollout="bot", bot_players=-1), dict(rollout="bot", bot_players=[0.5]), dict(rollout="bot", bot_random_permille=1001),
                dict(rollout="bot", bot_random_permille=-1), dict(rollout="bot", bot_random_permille=0.5),
                dict(rollout="bot", bot_random_permille=True)):
        with pytest.raises(ValueError):
            PlayoutSearch(_engine(), **bad)


def test_the_front_carries_the_setting_to_the_engine(monkeypatch):
    """evaluate() hands the engine the seat mask and the mix exactly when rollout is "bot"; the tensors are CPU ones here, so the
    device check is stood in for."""
    from generalsreinforcementlearning_amd import PlayoutSearch
    cand, players = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    for kw, want in ((dict(), {}), (dict(rollout="bot"), dict(bot_players=0b1111, bot_random_permille=0)),
                     (dict(rollout="bot", bot_players=[2], bot_random_permille=300), dict(bot_players=0b100, bot_random_permille=300))):
        eng = _engine()
        s = PlayoutSearch(eng, candidates=3, replicas=2, depth=4, **kw)
        monkeypatch.setattr(s, "_device", lambda: torch.device("cpu"))
        terms = s.evaluate(None, players, cand, seed=7)
        assert tuple(terms.shape) == (2, 3, 2, 8) and len(eng.calls) == 1
        a, got = eng.calls[0]
        assert a[0] == 2 and a[4:8] == (3, 2, 4, 7) and got == want


def test_search_playouts_device_picks_the_entry_point():
    """with both bot arguments at their defaults the existing entry point is called, with either one set the new one"""
    from generalsreinforcementlearning_amd import search
    seen = []

    class _Lib:
        def gvec_search_playouts(self, h, a):
            seen.append(("agent",))
            return 0

        def gvec_search_playouts_bot(self, h, a, players, permille):
            seen.append(("bot", players, permille))
            return 0

    eng = types.SimpleNamespace(L=_Lib(), h=None)
    search.search_playouts_device(eng, 1, 16, 16, 16, 2, 2, 2)
    search.search_playouts_device(eng, 1, 16, 16, 16, 2, 2, 2, bot_players=0, bot_random_permille=0)
    search.search_playouts_device(eng, 1, 16, 16, 16, 2, 2, 2, bot_players=0b10)
    search.search_playouts_device(eng, 1, 16, 16, 16, 2, 2, 2, bot_random_permille=40)
    assert seen == [("agent",), ("agent",), ("bot", 0b10, 0), ("bot", 0, 40)]
    with pytest.raises(ValueError):
        search.search_playouts_device(eng, 1, 16, 16, 16, 2, 2, 2, bot_players=-1)
    import inspect
    from generalsreinforcementlearning_amd import VecEngine
    p = inspect.signature(VecEngine.search_playouts_device).parameters
    assert p["bot_players"].default == 0 and p["bot_random_permille"].default == 0
