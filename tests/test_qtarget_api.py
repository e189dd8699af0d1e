"""The argument checks of gvec_obs_valid_mask, gvec_q_target and gvec_categorical_target and of their Python front
(q_targets.py).  The file runs with and without a device and its pointers are placeholders, so every call of an entry point
goes through tests/_api_calls.py, which launches nothing on them.

The checks that all five observation-batch entry points of gvec_api_obs.hip share (null arguments, rows, board, row stride,
zero rows, the bounds, valid arguments reaching the device) are one table here, ENTRY / REQUIRED / OPTIONAL, which also
lists gvec_obs_features and gvec_obs_memory_update; what only those two check is in test_features_api.py and
test_memory_api.py."""
import ctypes as C

import pytest

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


P = 1 << 20   # stands for a device pointer: no check dereferences it, a launch would (passes_checks keeps it from one)


def _mask_args(**over):
    kw = dict(rows=3, width=15, height=15, obs_row_stride=9 * 225, obs=P, mask=2 * P)
    kw.update(over)
    return lib.ObsValidMaskArgs(**kw)


def _q_args(**over):
    kw = dict(rows=3, width=15, height=15, obs_row_stride=9 * 225, gamma=0.99, reserved=0, next_obs=P, q_eval=2 * P, q_select=None,
              reward=3 * P, discount=None, done=4 * P, target=5 * P, next_action=6 * P, next_value=None)
    kw.update(over)
    return lib.QTargetArgs(**kw)


def _c_args(**over):
    kw = dict(rows=3, width=15, height=15, obs_row_stride=9 * 225, num_atoms=51, gamma=0.99, v_min=-10.0, v_max=10.0, next_obs=P,
              logits_eval=2 * P, logits_select=None, reward=3 * P, discount=None, done=4 * P, m=5 * P, next_action=6 * P)
    kw.update(over)
    return lib.CategoricalTargetArgs(**kw)


def _feat_args(**over):
    kw = dict(rows=3, width=15, height=15, cap=64, reserved=0, obs_row_stride=9 * 225, obs=P, out=2 * P)
    kw.update(over)
    return lib.ObsFeaturesArgs(**kw)


def _mem_args(**over):
    kw = dict(rows=3, width=15, height=15, cap=64, rows_per_flag=1, obs_row_stride=9 * 225, obs=P, prev=None, reset=None, out=2 * P)
    kw.update(over)
    return lib.ObsMemoryArgs(**kw)


ENTRY = {"gvec_obs_valid_mask": _mask_args, "gvec_q_target": _q_args, "gvec_categorical_target": _c_args,
         "gvec_obs_features": _feat_args, "gvec_obs_memory_update": _mem_args}
REQUIRED = {"gvec_obs_valid_mask": ("obs", "mask"),
            "gvec_q_target": ("next_obs", "q_eval", "reward", "done", "target", "next_action"),
            "gvec_categorical_target": ("next_obs", "logits_eval", "reward", "done", "m", "next_action"),
            "gvec_obs_features": ("obs", "out"), "gvec_obs_memory_update": ("obs", "out")}
OPTIONAL = {"gvec_obs_valid_mask": (), "gvec_q_target": ("q_select", "discount", "next_value"),
            "gvec_categorical_target": ("logits_select", "discount"), "gvec_obs_features": (),
            "gvec_obs_memory_update": ("prev", "reset")}


def _rejected(L, fn, a, text):
    rejected(L, fn, a, text)


def test_struct_layouts_match_the_header():
    f = lib.ObsValidMaskArgs
    assert C.sizeof(f) == 40
    assert (f.rows.offset, f.width.offset, f.height.offset, f.obs_row_stride.offset, f.obs.offset, f.mask.offset) == (0, 8, 12, 16, 24, 32)
    f = lib.QTargetArgs
    assert C.sizeof(f) == 104
    assert (f.rows.offset, f.width.offset, f.height.offset, f.obs_row_stride.offset, f.gamma.offset, f.reserved.offset, f.next_obs.offset,
            f.q_eval.offset, f.q_select.offset, f.reward.offset, f.discount.offset, f.done.offset, f.target.offset, f.next_action.offset,
            f.next_value.offset) == (0, 8, 12, 16, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96)
    f = lib.CategoricalTargetArgs
    assert C.sizeof(f) == 104
    assert (f.rows.offset, f.width.offset, f.height.offset, f.obs_row_stride.offset, f.num_atoms.offset, f.gamma.offset, f.v_min.offset,
            f.v_max.offset, f.next_obs.offset, f.logits_eval.offset, f.logits_select.offset, f.reward.offset, f.discount.offset,
            f.done.offset, f.m.offset, f.next_action.offset) == (0, 8, 12, 16, 24, 28, 32, 36, 40, 48, 56, 64, 72, 80, 88, 96)


@pytest.mark.parametrize("fn", ENTRY)
def test_null_arguments(L, fn):
    _rejected(L, fn, None, "args or a required pointer is NULL")
    for name in REQUIRED[fn]:
        _rejected(L, fn, ENTRY[fn](**{name: None}), "args or a required pointer is NULL")


@pytest.mark.parametrize("fn", ENTRY)
@pytest.mark.parametrize("rows", [-1, 2 ** 31, 2 ** 40])
def test_rows_out_of_range(L, fn, rows):
    _rejected(L, fn, ENTRY[fn](rows=rows), f"rows {rows} outside [0, 2^31)")


@pytest.mark.parametrize("fn", ENTRY)
@pytest.mark.parametrize("w,h", [(0, 15), (33, 15), (15, 0), (15, 33), (-1, 15)])
def test_board_out_of_range(L, fn, w, h):
    _rejected(L, fn, ENTRY[fn](width=w, height=h, obs_row_stride=9 * 33 * 33), "outside [1, 32]")


@pytest.mark.parametrize("fn", ENTRY)
def test_row_stride_too_small(L, fn):
    _rejected(L, fn, ENTRY[fn](obs_row_stride=9 * 225 - 1), "obs_row_stride 2024 < 9 * width * height = 2025")
    _rejected(L, fn, ENTRY[fn](obs_row_stride=0), "obs_row_stride 0 <")


def test_reserved_must_be_zero(L):
    _rejected(L, "gvec_q_target", _q_args(reserved=1), "reserved 1 must be 0")


@pytest.mark.parametrize("n", [-1, 0, 1, 65, 1024])
def test_num_atoms_out_of_range(L, n):
    _rejected(L, "gvec_categorical_target", _c_args(num_atoms=n), f"num_atoms {n} outside [2, 64]")


@pytest.mark.parametrize("lo,hi", [(1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")), (float("-inf"), 1.0),
                                   (0.0, float("inf"))])
def test_support_bounds(L, lo, hi):
    _rejected(L, "gvec_categorical_target", _c_args(v_min=lo, v_max=hi), "must be finite with v_min < v_max")


@pytest.mark.parametrize("fn", ENTRY)
def test_zero_rows_is_a_no_op_without_a_device(L, fn):
    passes_checks(L, fn, ENTRY[fn](rows=0))
    _rejected(L, fn, ENTRY[fn](rows=0, width=33), "outside [1, 32]")                 # the checks come first all the same
    _rejected(L, fn, ENTRY[fn](rows=0, **{REQUIRED[fn][0]: None}), "NULL")


def test_every_bound_is_accepted(L):
    """the extremes of every range pass the checks: rows == 0 keeps the call off the device"""
    for w, h in ((1, 1), (32, 32), (32, 1), (1, 32)):
        for fn in ENTRY:
            passes_checks(L, fn, ENTRY[fn](rows=0, width=w, height=h, obs_row_stride=9 * w * h))
    for n in (2, 64):
        passes_checks(L, "gvec_categorical_target", _c_args(rows=0, num_atoms=n, v_min=-1e30, v_max=1e30))


@pytest.mark.parametrize("fn", ENTRY)
def test_passing_arguments_reach_the_device_check(L, fn):
    """valid arguments, the optional pointers given or not, pass every check: what refuses them on a box without a GPU is the
    device, with another code"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    passes_checks(L, fn, ENTRY[fn]())                                                 # GVEC_E_NO_DEVICE
    passes_checks(L, fn, ENTRY[fn](obs_row_stride=9 * 225 + 7, **{k: 7 * P for k in OPTIONAL[fn]}))


def test_python_front_rejects_bad_input_before_any_launch():
    import torch
    from generalsreinforcementlearning_amd import categorical_target, double_q_target, valid_actions_mask_from_observation
    ns, q, lg = torch.zeros(4, 9, 5, 6), torch.zeros(4, 150), torch.zeros(4, 150, 51)
    r, d = torch.zeros(4), torch.zeros(4, dtype=torch.bool)
    # everything right but the device: the last check, so that the others are reachable on a box without a GPU
    for call in (lambda: valid_actions_mask_from_observation(ns), lambda: double_q_target(ns, q, r, 0.99, d),
                 lambda: double_q_target(ns, q, r.double(), r, d.to(torch.uint8), q_select=q),
                 lambda: categorical_target(ns, lg, r, 0.99, d, -10, 10),
                 lambda: categorical_target(ns, lg, r.half(), r, d, -10, 10, logits_select=lg)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    # the observation
    for fn in (valid_actions_mask_from_observation, lambda o: double_q_target(o, q, r, 0.99, d),
               lambda o: categorical_target(o, lg, r, 0.99, d, -10, 10)):
        with pytest.raises(TypeError, match="torch.Tensor"):
            fn([[0.0]])
        with pytest.raises(TypeError, match="float32"):
            fn(ns.double())
        for shape in ((4, 8, 5, 6), (4, 10, 5, 6), (9, 5), (5, 6)):
            with pytest.raises(ValueError, match=r"is not \[..., 9, H, W\]"):
                fn(torch.zeros(shape))
        with pytest.raises(ValueError, match=r"\[1, 32\]"):
            fn(torch.zeros(1, 9, 33, 5))
    # Q values and logits: dtype, and the observation's 5 * H * W
    with pytest.raises(TypeError, match="q_eval must be float32"):
        double_q_target(ns, q.double(), r, 0.99, d)
    with pytest.raises(TypeError, match="q_select must be float32"):
        double_q_target(ns, q, r, 0.99, d, q_select=q.half())
    for bad in (torch.zeros(4, 149), torch.zeros(4, 30), torch.zeros(3, 150), torch.zeros(4, 5, 30)):
        with pytest.raises(ValueError, match="q_eval .* is not"):
            double_q_target(ns, bad, r, 0.99, d)
        with pytest.raises(ValueError, match="q_select .* is not"):
            double_q_target(ns, q, r, 0.99, d, q_select=bad)
    with pytest.raises(TypeError, match="logits_eval must be float32"):
        categorical_target(ns, lg.double(), r, 0.99, d, -10, 10)
    for bad in (torch.zeros(4, 149, 51), torch.zeros(4, 150), torch.zeros(3, 150, 51), torch.zeros(4, 51, 150)):
        with pytest.raises(ValueError, match="logits_eval .* is not"):
            categorical_target(ns, bad, r, 0.99, d, -10, 10)
    with pytest.raises(ValueError, match="logits_select .* is not"):
        categorical_target(ns, lg, r, 0.99, d, -10, 10, logits_select=torch.zeros(4, 150, 50))
    # atoms and bounds
    for n in (1, 65):
        with pytest.raises(ValueError, match=r"num_atoms must be in \[2, 64\]"):
            categorical_target(ns, torch.zeros(4, 150, n), r, 0.99, d, -10, 10)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0)):
        with pytest.raises(ValueError, match="finite with v_min < v_max"):
            categorical_target(ns, lg, r, 0.99, d, lo, hi)
    # reward, discount, done
    for fn in (lambda **k: double_q_target(ns, q, **k), lambda **k: categorical_target(ns, lg, v_min=-10, v_max=10, **k)):
        with pytest.raises(TypeError, match="reward must be a floating-point"):
            fn(reward=torch.zeros(4, dtype=torch.int64), discount=0.99, done=d)
        with pytest.raises(ValueError, match="reward .* is not"):
            fn(reward=torch.zeros(5), discount=0.99, done=d)
        with pytest.raises(TypeError, match="discount must be a float or a tensor"):
            fn(reward=r, discount="0.99", done=d)
        with pytest.raises(TypeError, match="discount must be a floating-point"):
            fn(reward=r, discount=torch.ones(4, dtype=torch.int32), done=d)
        with pytest.raises(ValueError, match="discount .* is not"):
            fn(reward=r, discount=torch.ones(4, 1), done=d)
        with pytest.raises(TypeError, match="done must be bool or uint8"):
            fn(reward=r, discount=0.99, done=torch.zeros(4))
        with pytest.raises(ValueError, match="done .* is not"):
            fn(reward=r, discount=0.99, done=torch.zeros(3, dtype=torch.bool))
        with pytest.raises(TypeError, match="done must be a torch.Tensor"):
            fn(reward=r, discount=0.99, done=[0, 0, 0, 0])
