"""The two ways an argument-check test (tests/test_*_api.py) may call a gvec_* entry point.

Those tests hand the entry points integers that stand for device pointers.  That is sound as long as no kernel is launched on
them: a refused call returns before the device is looked at, and so does one with rows == 0.  A call that passes every check
with rows > 0 is launched when a device is present - asynchronously, on addresses nobody allocated, with return code 0 - and
the fault it causes surfaces in whatever synchronises next.  So such a call is made only where there is no device; accepted
arguments are run on real memory by the gpu-marked tests (test_hip_symmetry.py and test_hip_memory.py: touching buffers).
tests/test_api_calls.py keeps the test_*_api.py modules on these two functions."""
import ctypes as C

OK, E_INVALID, E_NO_DEVICE = 0, -1, -2               # GVEC_OK, GVEC_E_INVALID, GVEC_E_NO_DEVICE


def device_present():
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


def _call(L, fn, args):
    return getattr(L, fn)(0, None, C.byref(args) if args is not None else None)


def rejected(L, fn, args, text):
    """the call is refused with GVEC_E_INVALID and a message of fn's that holds text; args None is the null struct"""
    rc = _call(L, fn, args)
    msg = L.gvec_last_error().decode()
    assert rc == E_INVALID, (fn, rc, msg)
    assert text in msg and msg.startswith(fn + ":"), msg


def passes_checks(L, fn, args):
    """args pass every argument check of fn.  With rows == 0 the call returns 0 before it looks for a device.  With rows > 0
    it is made only on a box without a device, where it must get as far as the device check and no further (exactly
    GVEC_E_NO_DEVICE); with a device present it is NOT made, and the function returns (it does not skip, so that the
    rejections around it in the same test still run there)."""
    if args.rows == 0:
        rc = _call(L, fn, args)
        assert rc == OK, (fn, rc, L.gvec_last_error())
    elif not device_present():
        rc = _call(L, fn, args)
        assert rc == E_NO_DEVICE, (fn, rc, L.gvec_last_error())
