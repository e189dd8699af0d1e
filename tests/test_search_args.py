"""gvec_search_playouts names the field it refuses.  No GPU is needed, and none is used where there is one: every call here
passes a NULL handle, which the entry point looks at LAST - after every check of the arguments - so a call whose fields all
pass is refused for the handle, and no call can reach a launch on the placeholder pointers."""
import ctypes as C

import pytest

from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

FN = "gvec_search_playouts"
P = 4096            # a placeholder for a device pointer: never dereferenced (the handle is NULL)


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


def _args(**kw):
    a = dict(num_roots=4, num_candidates=3, replicas=2, depth=5, root_envs=None, root_players=P, candidates=P, seed=1, terms=P)
    a.update(kw)
    return lib.SearchArgs(**a)


def _refused(L, args, text):
    rc = L.gvec_search_playouts(None, C.byref(args) if args is not None else None)
    msg = L.gvec_last_error().decode()
    assert rc == -1, (rc, msg)                                               # GVEC_E_INVALID
    assert msg.startswith(FN + ":") and text in msg, msg


def test_null_args_and_null_handle(L):
    _refused(L, None, "args is NULL")
    _refused(L, _args(), "h is NULL")                                        # every field passes: the handle is what is missing
    _refused(L, _args(num_roots=0), "h is NULL")                             # ... for the no-op too
    _refused(L, _args(root_envs=P), "h is NULL")


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
