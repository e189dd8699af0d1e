"""The argument checks of gvec_obs_features and of its Python front (features.strategic_features, the envs' option).  The
file runs with and without a device and its pointers are placeholders, so every call of the entry point goes through
tests/_api_calls.py, which launches nothing on them.  The checks it shares with the other observation-batch entry points (null
arguments, rows, board, row stride) are in test_qtarget_api.py's table."""
import ctypes as C

import pytest

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


FN = "gvec_obs_features"
P = 4096   # stands for a device pointer: no check dereferences it, a launch would (passes_checks keeps it from one)


def _args(**over):
    kw = dict(rows=3, width=15, height=15, cap=64, reserved=0, obs_row_stride=9 * 225, obs=P, out=P)
    kw.update(over)
    return lib.ObsFeaturesArgs(**kw)


def _rejected(L, a, text):
    rejected(L, FN, a, text)


def test_struct_layout_matches_the_header():
    assert C.sizeof(lib.ObsFeaturesArgs) == 48
    f = lib.ObsFeaturesArgs
    assert (f.rows.offset, f.width.offset, f.height.offset, f.cap.offset, f.reserved.offset, f.obs_row_stride.offset, f.obs.offset,
            f.out.offset) == (0, 8, 12, 16, 20, 24, 32, 40)


@pytest.mark.parametrize("cap", [0, 1, 3, 48, 2048, -64])
def test_cap_not_a_power_of_two_in_range(L, cap):
    _rejected(L, _args(cap=cap), f"cap {cap} is not a power of two in [2, 1024]")


def test_reserved_must_be_zero(L):
    _rejected(L, _args(reserved=1), "reserved 1 must be 0")


def test_zero_rows_is_a_no_op_without_a_device(L):
    passes_checks(L, FN, _args(rows=0))
    passes_checks(L, FN, _args(rows=0, obs_row_stride=9 * 225 + 7, cap=1024))
    _rejected(L, _args(rows=0, cap=48), "cap 48")                       # the checks come first all the same


def test_every_bound_is_accepted(L):
    """the extremes of every range pass the checks: rows == 0 keeps the call off the device"""
    for w, h, cap in ((1, 1, 2), (32, 32, 1024), (32, 1, 2), (1, 32, 1024)):
        passes_checks(L, FN, _args(rows=0, width=w, height=h, cap=cap, obs_row_stride=9 * w * h))


def test_strategic_features_rejects_bad_input_before_any_launch():
    import torch
    from generalsreinforcementlearning_amd import NUM_STRATEGIC_FEATURES, STRATEGIC_FEATURE_NAMES, strategic_features
    assert NUM_STRATEGIC_FEATURES == 5 == len(STRATEGIC_FEATURE_NAMES)
    with pytest.raises((ValueError, TypeError)):
        strategic_features(torch.zeros(2, 9, 5, 5))                      # a CPU tensor
    with pytest.raises((ValueError, TypeError)):
        strategic_features(torch.zeros(2, 9, 5, 5, dtype=torch.float64))
    with pytest.raises((ValueError, TypeError)):
        strategic_features(torch.zeros(2, 8, 5, 5))
    with pytest.raises((ValueError, TypeError)):
        strategic_features(torch.zeros(2, 9, 5, 5), cap=48)
    with pytest.raises((ValueError, TypeError)):
        strategic_features(torch.zeros(2, 9, 5, 5), cap=64.0)
    with pytest.raises((ValueError, TypeError)):
        strategic_features([[0.0]])
    assert "not differentiable" in strategic_features.__doc__


def test_row_stride_detection():
    """which layouts are read in place (no copy) and which fall back to .contiguous()"""
    import torch
    from generalsreinforcementlearning_amd._obs_batch import row_stride as _row_stride
    n = 9 * 4 * 5
    x = torch.zeros(6, 2, 9, 4, 5)
    assert _row_stride(x, 3, n) == n
    assert _row_stride(x[:, 0], 3, n) == 2 * n                            # one learner of every env: a common stride
    assert _row_stride(x[::2], 3, n) is None                              # [3, 2] with strides (4n, n): no common stride
    assert _row_stride(x[::2, 0], 3, n) == 4 * n
    assert _row_stride(x[..., :3], 3, 9 * 4 * 3) is None                  # planes not dense
    big = torch.zeros(7, n + 11)
    assert _row_stride(big[:, :n].view(7, 9, 4, 5), 3, n) == n + 11
    assert _row_stride(x[:1].expand(4, 2, 9, 4, 5), 3, n) is None         # stride 0
    assert _row_stride(torch.zeros(9, 4, 5), 3, n) == n
    assert _row_stride(torch.zeros(3, 9, 20), 2, n) == n


@pytest.mark.parametrize("cls", ["GeneralsVecEnv", "GeneralsSelfPlayVecEnv"])
def test_env_option_needs_device_outputs(cls):
    import generalsreinforcementlearning_amd.selfplay_env as sp
    import generalsreinforcementlearning_amd.vector_env as ve
    env = getattr(ve if cls == "GeneralsVecEnv" else sp, cls)
    with pytest.raises(ValueError, match="device_outputs"):
        env(4, 8, 8, strategic_features=True)
    with pytest.raises(ValueError, match="power of two"):
        env(4, 8, 8, device_outputs=True, strategic_features=True, feature_cap=48)
