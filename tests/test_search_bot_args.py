"""gvec_search_playouts_bot names the argument it refuses.  No GPU is needed, and none is used where there is one: every call
here passes a NULL handle, which the entry point looks at LAST - after every check of the arguments - so a call whose
arguments all pass is refused for the handle, and no call can reach a launch on the placeholder pointers.  (The method of
tests/test_search_args.py, whose every case is repeated here under the new name: both entry points make the struct's
checks through one helper.)"""
import ctypes as C

import pytest

from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

FN = "gvec_search_playouts_bot"
P = 4096            # a placeholder for a device pointer: never dereferenced (the handle is NULL)


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


def _args(**kw):
    a = dict(num_roots=4, num_candidates=3, replicas=2, depth=5, root_envs=None, root_players=P, candidates=P, seed=1, terms=P)
    a.update(kw)
    return lib.SearchArgs(**a)


def _refused(L, args, text, bot_players=0b11, permille=0):
    rc = L.gvec_search_playouts_bot(None, C.byref(args) if args is not None else None, bot_players, permille)
    msg = L.gvec_last_error().decode()
    assert rc == -1, (rc, msg)                                               # GVEC_E_INVALID
    assert msg.startswith(FN + ":") and text in msg, msg


def test_null_args_and_null_handle(L):
    _refused(L, None, "args is NULL")
    _refused(L, _args(), "h is NULL")                                        # every argument passes: the handle is what is missing
    _refused(L, _args(num_roots=0), "h is NULL")                             # ... for the no-op too
    _refused(L, _args(root_envs=P), "h is NULL")
    _refused(L, _args(), "h is NULL", bot_players=0)                         # no seat on the rule is legal
    _refused(L, _args(), "h is NULL", bot_players=0xFF, permille=1000)       # every seat of the largest handle, the agent's move always


@pytest.mark.parametrize("field,value,text", [
    ("root_players", None, "root_players is NULL"), ("candidates", None, "candidates is NULL"), ("terms", None, "terms is NULL"),
    ("num_roots", -1, "num_roots -1"), ("num_candidates", 0, "num_candidates 0"), ("replicas", 0, "replicas 0"), ("depth", 0, "depth 0"),
    ("num_candidates", -5, "num_candidates -5"), ("depth", -1, "depth -1")])
def test_each_field_is_named_when_refused(L, field, value, text):
    _refused(L, _args(**{field: value}), text)


def test_too_many_playouts_are_refused(L):
    _refused(L, _args(num_roots=2 ** 20, num_candidates=2 ** 10, replicas=2), "2^31")
    _refused(L, _args(num_roots=1, num_candidates=2 ** 16, replicas=2 ** 16), "2^31")      # K * R alone overflows int32
    _refused(L, _args(num_roots=2 ** 20, num_candidates=2 ** 10, replicas=1), "h is NULL")  # 2^30 playouts pass the count check


@pytest.mark.parametrize("permille", [-1, 1001, 2 ** 31 - 1, -2 ** 31])
def test_the_mix_outside_its_range_is_refused(L, permille):
    _refused(L, _args(), "bot_random_permille must be in [0, 1000]", permille=permille)


@pytest.mark.parametrize("mask", [1 << 8, 1 << 31, 0xFFFFFFFF, 0x1FF])
def test_a_seat_no_handle_has_is_refused(L, mask):
    """GVEC_MAX_PLAYERS is 8: a bit at or above it names a seat at or above any handle's max_players, which needs no handle
    to know (a bit below it is checked against the handle's own max_players: tests/test_hip_search_bot.py)."""
    _refused(L, _args(), "bot_players names a seat at or above max_players", bot_players=mask)


def test_the_structs_checks_come_first_and_the_handle_last(L):
    _refused(L, _args(depth=0), "depth 0", bot_players=1 << 8, permille=-1)
    _refused(L, _args(), "bot_random_permille", bot_players=1 << 8, permille=-1)
