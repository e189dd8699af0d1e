"""Keeps the argument-check modules (tests/test_*_api.py) on the two functions of tests/_api_calls.py, and pins those two."""
import ast
import ctypes as C
import glob
import os

import pytest

import _api_calls as AC

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_ONLY = {"gvec_last_error", "gvec_abi_version"}          # take no pointer of the caller's and launch nothing


def direct_entry_point_calls(source, filename="<source>"):
    """(line, what) of every place where a module reaches a gvec_* entry point by itself"""
    found = []
    for node in ast.walk(ast.parse(source, filename)):
        if isinstance(node, ast.Attribute) and node.attr.startswith("gvec_") and node.attr not in HOST_ONLY:
            found.append((node.lineno, "." + node.attr))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Call) and isinstance(node.func.func, ast.Name) \
                and node.func.func.id == "getattr":
            found.append((node.lineno, "getattr(...)(...)"))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr" and len(node.args) >= 2 \
                and isinstance(node.args[1], ast.Constant) and isinstance(node.args[1].value, str) \
                and node.args[1].value.startswith("gvec_") and node.args[1].value not in HOST_ONLY:
            found.append((node.lineno, f"getattr(..., {node.args[1].value!r})"))
    return sorted(found)


def _api_modules():
    return sorted(glob.glob(os.path.join(HERE, "test_*_api.py")))


def test_api_modules_call_entry_points_through_the_helpers_only():
    """The rule: a tests/test_*_api.py module hands placeholder integers to the library as device pointers, so it reaches a
    gvec_* entry point through _api_calls.rejected or _api_calls.passes_checks and in no other way.  Read off the syntax tree,
    that is: no attribute gvec_<name> of any object (which covers L.gvec_x(...), lib.load().gvec_x and f = L.gvec_x), no
    getattr(...) whose result is called on the spot, and no getattr(..., "gvec_<name>").  What this does not see: a getattr
    with a computed name whose result is first bound to a variable.  Functions of the host that take no pointer of the
    caller's (HOST_ONLY) and everything that is no entry point - struct layouts, the Python fronts on CPU tensors - stay direct.
    A new module of the kind, named test_<subsystem>_api.py like these, is covered from its first commit."""
    modules = _api_modules()
    assert {os.path.basename(m) for m in modules} >= {"test_symmetry_api.py", "test_memory_api.py", "test_features_api.py",
                                                      "test_qtarget_api.py", "test_arena_api.py"}
    bad = []
    for path in modules:
        with open(path) as f:
            bad += [f"{os.path.basename(path)}:{line}: {what}" for line, what in direct_entry_point_calls(f.read(), path)]
    assert not bad, "entry points called past tests/_api_calls.py:\n" + "\n".join(bad)


def test_the_scan_sees_each_spelling():
    scan = lambda src: [what for _, what in direct_entry_point_calls(src)]                                  # noqa: E731
    assert scan("assert L.gvec_obs_symmetry(0, None, C.byref(_args(applied=P + 3))) != -1\n") == [".gvec_obs_symmetry"]
    assert scan("f = lib.load().gvec_q_target\nf(0, None, a)\n") == [".gvec_q_target"]
    assert scan("rc = getattr(L, fn)(0, None, C.byref(a))\n") == ["getattr(...)(...)"]
    assert scan("f = getattr(L, 'gvec_arena_update')\n") == ["getattr(..., 'gvec_arena_update')"]
    assert scan("passes_checks(L, FN, _args(rows=0))\nmsg = L.gvec_last_error()\nenv = getattr(ve, cls)\nenv(4, 8, 8)\n") == []


# ---- the two helpers themselves, on a stand-in library: what they assert, and that one of them does not call ---------------

class _Args(C.Structure):
    _fields_ = [("rows", C.c_int64)]


class _FakeLib:
    def __init__(self, rc, msg=b""):
        self.rc, self.msg, self.calls = rc, msg, 0

    def gvec_fake(self, device, stream, args):
        self.calls += 1
        return self.rc

    def gvec_last_error(self):
        return self.msg


def test_rejected_wants_minus_one_and_the_entry_points_own_message():
    AC.rejected(_FakeLib(-1, b"gvec_fake: rows -1 outside"), "gvec_fake", _Args(rows=-1), "rows -1")
    AC.rejected(_FakeLib(-1, b"gvec_fake: NULL"), "gvec_fake", None, "NULL")
    for lib in (_FakeLib(0, b"gvec_fake: rows -1"), _FakeLib(-2, b"gvec_fake: rows -1"), _FakeLib(-1, b"gvec_other: rows -1"),
                _FakeLib(-1, b"gvec_fake: something else")):
        with pytest.raises(AssertionError):
            AC.rejected(lib, "gvec_fake", _Args(rows=-1), "rows -1")


@pytest.mark.parametrize("device", [False, True])
def test_passes_checks_launches_nothing_where_a_device_is(monkeypatch, device):
    monkeypatch.setattr(AC, "device_present", lambda: device)
    lib = _FakeLib(0)
    AC.passes_checks(lib, "gvec_fake", _Args(rows=0))                    # rows == 0: called wherever it runs, and 0
    assert lib.calls == 1
    for rc in (-1, -2):
        with pytest.raises(AssertionError):
            AC.passes_checks(_FakeLib(rc), "gvec_fake", _Args(rows=0))
    lib = _FakeLib(-2)
    AC.passes_checks(lib, "gvec_fake", _Args(rows=3))
    assert lib.calls == (0 if device else 1)                             # with a device: not called at all
    for rc in (0, -1, -3):
        lib = _FakeLib(rc)
        if device:
            AC.passes_checks(lib, "gvec_fake", _Args(rows=3))
            assert lib.calls == 0
        else:
            with pytest.raises(AssertionError):                          # exactly GVEC_E_NO_DEVICE, nothing else
                AC.passes_checks(lib, "gvec_fake", _Args(rows=3))
