"""The argument checks of gvec_obs_memory_update and of its Python front (memory.ObservationMemory).  The file runs with and
without a device and its pointers are placeholders, so every call of the entry point goes through tests/_api_calls.py: one
that passes the checks with rows > 0 is made only where no device can launch it (test_hip_memory.py runs such arguments on
real memory).  The checks it shares with the other observation-batch entry points (null arguments, rows, board, row stride)
are in test_qtarget_api.py's table."""
import ctypes as C

import pytest

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


FN = "gvec_obs_memory_update"
P = 1 << 20   # stands for a device pointer: no check dereferences it, a launch would (passes_checks keeps it from one)
STATE = 3 * 4 * 225 * 4   # bytes of the default arguments' state


def _args(**over):
    kw = dict(rows=3, width=15, height=15, cap=64, rows_per_flag=1, obs_row_stride=9 * 225, obs=P, prev=None, reset=None, out=2 * P)
    kw.update(over)
    return lib.ObsMemoryArgs(**kw)


def _rejected(L, a, text):
    rejected(L, FN, a, text)


def test_struct_layout_matches_the_header():
    assert C.sizeof(lib.ObsMemoryArgs) == 64
    f = lib.ObsMemoryArgs
    assert (f.rows.offset, f.width.offset, f.height.offset, f.cap.offset, f.rows_per_flag.offset, f.obs_row_stride.offset,
            f.obs.offset, f.prev.offset, f.reset.offset, f.out.offset) == (0, 8, 12, 16, 20, 24, 32, 40, 48, 56)


@pytest.mark.parametrize("cap", [0, 1, 3, 48, 2048, -64])
def test_cap_not_a_power_of_two_in_range(L, cap):
    _rejected(L, _args(cap=cap), f"cap {cap} is not a power of two in [2, 1024]")


@pytest.mark.parametrize("rows,rpf", [(3, 0), (3, -1), (3, 2), (4, 3), (0, 0)])
def test_rows_per_flag_must_divide_rows(L, rows, rpf):
    _rejected(L, _args(rows=rows, rows_per_flag=rpf), f"rows_per_flag {rpf} is not a divisor >= 1 of rows {rows}")


@pytest.mark.parametrize("delta", [4, -4, STATE - 4, 4 - STATE, 900])
def test_prev_overlapping_out_without_being_it(L, delta):
    _rejected(L, _args(prev=2 * P + delta), "prev overlaps out without being equal to it")


def test_zero_rows_is_a_no_op_without_a_device(L):
    passes_checks(L, FN, _args(rows=0))
    passes_checks(L, FN, _args(rows=0, rows_per_flag=7, obs_row_stride=9 * 225 + 7, cap=1024, prev=2 * P, reset=3 * P))
    _rejected(L, _args(rows=0, cap=48), "cap 48")                       # the checks come first all the same
    _rejected(L, _args(rows=0, out=None), "NULL")


def test_every_bound_is_accepted(L):
    """the extremes of every range pass the checks: rows == 0 keeps the call off the device"""
    for w, h, cap in ((1, 1, 2), (32, 32, 1024), (32, 1, 2), (1, 32, 1024)):
        passes_checks(L, FN, _args(rows=0, width=w, height=h, cap=cap, obs_row_stride=9 * w * h))


def test_passing_arguments_reach_the_device_check(L):
    """in place (prev == out) and buffers that merely touch pass every argument check: what refuses them on a box without a
    GPU is the device, with another code"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for prev in (2 * P, 2 * P + STATE, 2 * P - STATE):
        passes_checks(L, FN, _args(prev=prev))                                      # GVEC_E_NO_DEVICE


def test_python_front_rejects_bad_input_before_any_launch():
    import torch
    from generalsreinforcementlearning_amd import (MEMORY_PLANE_NAMES, NUM_MEMORY_PLANES, ObservationMemory,
                                                   remembered_observation)
    assert NUM_MEMORY_PLANES == 4 == len(MEMORY_PLANE_NAMES)
    assert MEMORY_PLANE_NAMES == ("seen", "last_owner", "last_army", "age")
    for cap in (48, 1, 2048):
        with pytest.raises(ValueError, match="power of two"):
            ObservationMemory((4, 2), 5, 5, cap=cap)
    with pytest.raises(TypeError):
        ObservationMemory((4, 2), 5, 5, cap=64.0)
    with pytest.raises(ValueError, match=r"\[1, 32\]"):
        ObservationMemory((4, 2), 33, 5)
    with pytest.raises(ValueError, match="rows_shape"):
        ObservationMemory((4, -2), 5, 5)
    with pytest.raises(ValueError, match="CUDA"):
        ObservationMemory((4, 2), 5, 5, device="cpu")
    m = ObservationMemory((4, 2), 5, 5)                                  # allocates nothing: fine without a device
    assert m.shape == (4, 2, 4, 5, 5) and m.rows == 8 and m.cap == 64
    good = torch.zeros(4, 2, 9, 5, 5)
    with pytest.raises(ValueError, match="CUDA"):
        m.update(good)                                                   # a CPU tensor
    with pytest.raises(TypeError, match="float32"):
        m.update(good.double())
    with pytest.raises(TypeError, match="torch.Tensor"):
        m.update([[0.0]])
    for shape in ((4, 2, 8, 5, 5), (8, 9, 5, 5), (4, 2, 9, 5, 6), (2, 4, 9, 5, 5)):
        with pytest.raises(ValueError, match="is not"):
            m.update(torch.zeros(shape))
    for shape in ((2,), (4, 1), (4, 2, 9), (8,)):
        with pytest.raises(ValueError, match="no leading prefix"):
            m.update(good, reset=torch.zeros(shape, dtype=torch.bool))
    with pytest.raises(TypeError, match="bool or uint8"):
        m.update(good, reset=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="torch.Tensor"):
        m.update(good, reset=[0, 0, 0, 0])
    with pytest.raises(ValueError):
        remembered_observation(torch.zeros(3, 9, 5, 5), torch.zeros(3, 5, 5, 5))
    with pytest.raises(ValueError):
        remembered_observation(torch.zeros(3, 9, 5, 5), torch.zeros(2, 4, 5, 5))
    obs, mem = torch.rand(3, 9, 5, 5), torch.rand(3, 4, 5, 5)           # plain torch: works wherever the tensors are
    r = remembered_observation(obs, mem)
    assert r.shape == (3, 9, 5, 5) and torch.equal(r[:, 0], obs[:, 0]) and torch.equal(r[:, 1:3], mem[:, 1:3])
    assert torch.equal(r[:, 3:], obs[:, 3:])


def test_rollout_buffer_refuses_a_memory_of_another_shape():
    from generalsreinforcementlearning_amd import ObservationMemory, SelfPlayRolloutBuffer

    class Env:                                                           # what the constructor reads before it allocates
        device_outputs, num_envs, num_learners, board_height, board_width = True, 4, 2, 5, 5
    for mem in (ObservationMemory((4, 3), 5, 5), ObservationMemory((8,), 5, 5), ObservationMemory((4, 2), 5, 6), object()):
        with pytest.raises(ValueError, match="ObservationMemory of rows_shape"):
            SelfPlayRolloutBuffer(Env(), 4, memory=mem)
