"""The argument checks of gvec_obs_symmetry and of its Python front (symmetry.py).  The file is not marked gpu, so it runs
on a box without a device and on one with a device alike, and its pointers are placeholders: every call of the entry point
goes through tests/_api_calls.py, which makes a call that passes the checks with rows > 0 only where no device can launch
it.  What such arguments compute is checked on real memory in test_hip_symmetry.py (touching buffers)."""
import ctypes as C

import pytest

from _api_calls import passes_checks, rejected
from generalsreinforcementlearning_amd import _lib as lib
from generalsreinforcementlearning_amd.csrc import build as B

FN = "gvec_obs_symmetry"


@pytest.fixture(scope="module")
def L():
    B.build(verbose=False)
    return lib.load()


# Stands for a device pointer.  No check dereferences it, but a launch would: a call that is accepted with rows > 0 goes
# through passes_checks.  Pointers P apart never overlap at these sizes
P = 1 << 24


def _args(sets=((9, 9 * 225),), **over):
    """3 rows of 15x15: the plane sets given as (planes, in_row_stride), and mask, values, action and applied"""
    kw = dict(rows=3, width=15, height=15, num_sets=len(sets), inverse=0, reserved=0, sym=P, mask_in=2 * P, mask_out=3 * P,
              values_in=4 * P, values_out=5 * P, action_in=6 * P, action_out=7 * P, applied=8 * P)
    kw.update(over)
    a = lib.ObsSymmetryArgs(**kw)
    for k, (planes, stride) in enumerate(sets):
        a.sets[k].in_, a.sets[k].out, a.sets[k].planes, a.sets[k].in_row_stride = (10 + 2 * k) * P, (11 + 2 * k) * P, planes, stride
    return a


def _rejected(L, a, text):
    rejected(L, FN, a, text)


def test_struct_layout_matches_the_header():
    s = lib.SymPlaneSet
    assert C.sizeof(s) == 32 and (s.in_.offset, s.out.offset, s.planes.offset, s.in_row_stride.offset) == (0, 8, 16, 24)
    f = lib.ObsSymmetryArgs
    assert C.sizeof(f) == 224
    assert (f.rows.offset, f.width.offset, f.height.offset, f.num_sets.offset, f.inverse.offset, f.reserved.offset, f.sets.offset,
            f.sym.offset, f.mask_in.offset, f.mask_out.offset, f.values_in.offset, f.values_out.offset, f.action_in.offset,
            f.action_out.offset, f.applied.offset) == (0, 8, 12, 16, 20, 24, 32, 160, 168, 176, 184, 192, 200, 208, 216)
    assert lib.SYM_MAX_PLANE_SETS == 4


def test_null_arguments(L):
    _rejected(L, None, "args or a required pointer is NULL")
    _rejected(L, _args(sym=None), "args or a required pointer is NULL")
    for half in ("mask_in", "mask_out", "values_in", "values_out", "action_in", "action_out"):      # a pair goes together
        _rejected(L, _args(**{half: None}), "args or a required pointer is NULL")
    for field in ("in_", "out"):
        a = _args(sets=((9, 2025), (4, 900)))
        setattr(a.sets[1], field, None)
        _rejected(L, a, "args or a required pointer is NULL")


def test_nothing_to_transform(L):
    nothing = dict(mask_in=None, mask_out=None, values_in=None, values_out=None, action_in=None, action_out=None)
    _rejected(L, _args(sets=(), **nothing), "nothing to transform")
    _rejected(L, _args(sets=(), applied=None, **nothing), "nothing to transform")
    for keep in ("mask", "values", "action"):            # any one of them is something
        some = {k: v for k, v in nothing.items() if not k.startswith(keep)}
        passes_checks(L, FN, _args(sets=(), rows=0, **some))


@pytest.mark.parametrize("rows", [-1, 2 ** 31, 2 ** 40])
def test_rows_out_of_range(L, rows):
    _rejected(L, _args(rows=rows), f"rows {rows} outside [0, 2^31)")


@pytest.mark.parametrize("w,h", [(0, 15), (33, 15), (15, 0), (15, 33), (-1, 15)])
def test_board_out_of_range(L, w, h):
    _rejected(L, _args(sets=((9, 9 * 33 * 33),), width=w, height=h), "outside [1, 32]")


def test_plane_sets(L):
    for n in (-1, 5):
        _rejected(L, _args(num_sets=n), f"num_sets {n} outside [0, 4]")
    for planes in (0, 65, -1):
        _rejected(L, _args(sets=((9, 2025), (planes, 65 * 225))), f"sets[1].planes {planes} outside [1, 64]")
    _rejected(L, _args(sets=((9, 9 * 225 - 1),)), "sets[0].in_row_stride 2024 < planes * width * height = 2025")
    _rejected(L, _args(sets=((9, 2025), (9, 2025), (4, 900), (5, 0))), "sets[3].in_row_stride 0 <")
    # the bounds themselves pass (rows == 0 keeps the call off the device)
    passes_checks(L, FN, _args(sets=((1, 225), (64, 64 * 225), (9, 2025 + 7), (5, 1125)), rows=0))


def test_inverse_and_reserved(L):
    for v in (-1, 2):
        _rejected(L, _args(inverse=v), f"inverse {v} is neither 0 nor 1")
    _rejected(L, _args(reserved=1), "reserved 1 must be 0")
    passes_checks(L, FN, _args(inverse=1, rows=0))


def test_an_output_may_not_overlap_an_input(L):
    # equal pointers: no tensor is transformed in place
    a = _args()
    a.sets[0].out = a.sets[0].in_
    _rejected(L, a, "output sets[0].out overlaps input sets[0].in")
    _rejected(L, _args(mask_out=2 * P), "output mask_out overlaps input mask_in")
    _rejected(L, _args(values_out=4 * P), "output values_out overlaps input values_in")
    _rejected(L, _args(action_out=6 * P), "output action_out overlaps input action_in")
    _rejected(L, _args(applied=P), "output applied overlaps input sym")
    # one output against another tensor's input, and partial overlap at either end: 3 rows of 9 * 225 floats are 24,300 bytes
    a = _args(sets=((9, 2025), (9, 2025)))
    a.sets[1].out = a.sets[0].in_
    _rejected(L, a, "output sets[1].out overlaps input sets[0].in")
    # (buffers that exactly touch are accepted: those calls would be launched, see passes_checks)
    for delta, ok in ((24299, False), (24300, True), (-24299, False), (-24300, True)):
        a = _args()
        a.sets[0].out = a.sets[0].in_ + delta
        if ok:
            passes_checks(L, FN, a)
        else:
            _rejected(L, a, "output sets[0].out overlaps input sets[0].in")
    # a strided input reaches as far as its last row: (rows - 1) * stride + planes * H * W floats
    a = _args(sets=((9, 4050),))
    a.sets[0].out = a.sets[0].in_ + (2 * 4050 + 2025) * 4 - 1
    _rejected(L, a, "output sets[0].out overlaps input sets[0].in")
    a.sets[0].out += 1
    passes_checks(L, FN, a)
    # the mask row is 1,125 bytes, sym one byte per row
    _rejected(L, _args(mask_out=2 * P + 3 * 1125 - 1), "output mask_out overlaps input mask_in")
    _rejected(L, _args(applied=P + 2), "output applied overlaps input sym")
    passes_checks(L, FN, _args(applied=P + 3))


def test_zero_rows_is_a_no_op_without_a_device(L):
    passes_checks(L, FN, _args(rows=0))
    _rejected(L, _args(rows=0, width=33), "outside [1, 32]")                         # the checks come first all the same
    _rejected(L, _args(rows=0, sym=None), "NULL")
    for w, h in ((1, 1), (32, 32), (32, 1), (1, 32)):
        passes_checks(L, FN, _args(sets=((9, 9 * w * h),), rows=0, width=w, height=h))


def test_passing_arguments_reach_the_device_check(L):
    """valid arguments pass every check: what refuses them on a box without a GPU is the device, with another code"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    passes_checks(L, FN, _args())                                                     # GVEC_E_NO_DEVICE
    passes_checks(L, FN, _args(sets=((9, 2025), (9, 2025 + 7), (4, 900), (5, 1125)), inverse=1))


def test_python_front_rejects_bad_input_before_any_launch():
    import torch
    from generalsreinforcementlearning_amd import (apply_symmetry, augment_transition, inverse_symmetry, num_symmetries,
                                                   random_symmetries)
    s, ns = torch.zeros(4, 9, 5, 6), torch.zeros(4, 9, 5, 6)
    mask, q, act = torch.zeros(4, 150, dtype=torch.bool), torch.zeros(4, 150), torch.zeros(4, dtype=torch.int64)
    sym = torch.zeros(4, dtype=torch.uint8)
    # everything right but the device: the last check, so that the others are reachable on a box without a GPU
    for call in (lambda: apply_symmetry(sym, s), lambda: apply_symmetry(sym, (s, ns), mask=mask, values=q, action=act),
                 lambda: apply_symmetry(1, s, mask=mask.to(torch.uint8), inverse=True, return_applied=True),
                 lambda: apply_symmetry(sym, values=q, height=5, width=6), lambda: apply_symmetry(3, action=act, height=5, width=6),
                 lambda: augment_transition(s, act, ns), lambda: augment_transition(s, act, ns, sym=sym),
                 lambda: augment_transition(s, act, ns, sym=2)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    # non-tensors and wrong dtypes
    with pytest.raises(TypeError, match="planes must be a torch.Tensor or a tuple"):
        apply_symmetry(sym, 3.0)
    with pytest.raises(TypeError, match=r"planes\[1\] must be a torch.Tensor"):
        apply_symmetry(sym, (s, [[0.0]]))
    with pytest.raises(TypeError, match=r"planes\[0\] must be float32"):
        apply_symmetry(sym, s.double())
    with pytest.raises(TypeError, match="mask must be bool or uint8"):
        apply_symmetry(sym, s, mask=q)
    with pytest.raises(TypeError, match="values must be float32"):
        apply_symmetry(sym, s, values=q.half())
    with pytest.raises(TypeError, match="action must be int64"):
        apply_symmetry(sym, s, action=act.int())
    with pytest.raises(TypeError, match="action must be a torch.Tensor"):
        apply_symmetry(sym, s, action=[0, 1, 2, 3])
    with pytest.raises(TypeError, match="sym must be uint8"):
        apply_symmetry(sym.long(), s)
    for bad in (1.0, "1", True, None):
        with pytest.raises(TypeError, match="sym must be a uint8 tensor or an int"):
            apply_symmetry(bad, s)
    with pytest.raises(TypeError, match="s must be float32"):
        augment_transition(s.double(), act, ns)
    with pytest.raises(TypeError, match="a must be int64"):
        augment_transition(s, act.int(), ns)
    # shapes that disagree
    for bad in (torch.zeros(5, 6), torch.zeros(4, 0, 5, 6), torch.zeros(4, 65, 5, 6)):
        with pytest.raises(ValueError, match=r"is not \[..., P, H, W\] with P in \[1, 64\]"):
            apply_symmetry(sym, bad)
    with pytest.raises(ValueError, match=r"\[1, 32\]"):
        apply_symmetry(sym, torch.zeros(4, 9, 33, 5))
    with pytest.raises(ValueError, match=r"planes\[0\] .* is not \(4, 'P', 5, 6\)"):
        apply_symmetry(sym, torch.zeros(3, 9, 5, 6))
    with pytest.raises(ValueError, match=r"planes\[1\] .* is not \(4, 'P', 5, 6\)"):
        apply_symmetry(sym, (s, torch.zeros(2, 2, 4, 5, 6)))
    with pytest.raises(ValueError, match=r"planes\[1\] .* is not on the 5x6 board"):
        apply_symmetry(sym, (s, torch.zeros(4, 4, 6, 5)))
    with pytest.raises(ValueError, match="is not on the 6x5 board"):
        apply_symmetry(sym, s, height=6, width=5)
    for bad in (torch.zeros(4, 149, dtype=torch.bool), torch.zeros(3, 150, dtype=torch.bool), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask .* is not"):
            apply_symmetry(sym, s, mask=bad)
    for bad in (torch.zeros(4, 151), torch.zeros(4, 5, 30)):
        with pytest.raises(ValueError, match="values .* is not"):
            apply_symmetry(sym, s, values=bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="action .* is not"):
            apply_symmetry(sym, s, action=bad)
        with pytest.raises(ValueError, match="action .* is not"):
            augment_transition(s, bad, ns, sym=sym)
    # the board, when no planes carry it
    with pytest.raises(ValueError, match="give height= and width="):
        apply_symmetry(sym, mask=mask)
    with pytest.raises(ValueError, match="height and width go together"):
        apply_symmetry(sym, mask=mask, height=5)
    # more than four plane sets, nothing to transform, an int sym the board does not have
    with pytest.raises(ValueError, match="5 plane sets: one call takes at most 4"):
        apply_symmetry(sym, (s,) * 5)
    with pytest.raises(ValueError, match="nothing to transform"):
        apply_symmetry(sym)
    with pytest.raises(ValueError, match="nothing to transform"):
        apply_symmetry(sym, (), height=5, width=6, return_applied=True)
    for bad in (4, 7, 8, -1):
        with pytest.raises(ValueError, match=f"sym {bad} is not one of the 4 symmetries of a 5x6 board"):
            apply_symmetry(bad, s)
    for bad in (8, -1):
        with pytest.raises(ValueError, match=f"sym {bad} is not one of the 8 symmetries of a 5x5 board"):
            apply_symmetry(bad, torch.zeros(4, 9, 5, 5))
    # the small helpers
    assert num_symmetries(5, 5) == 8 and num_symmetries(5, 6) == 4 and num_symmetries(1, 1) == 8
    with pytest.raises(ValueError, match=r"\[1, 32\]"):
        num_symmetries(0, 5)
    assert [inverse_symmetry(k) for k in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    inv = inverse_symmetry(torch.arange(8, dtype=torch.uint8))
    assert inv.dtype == torch.uint8 and inv.tolist() == [0, 1, 2, 3, 4, 6, 5, 7]
    for bad in (8, -1):
        with pytest.raises(ValueError, match=r"sym must be in \[0, 8\)"):
            inverse_symmetry(bad)
    with pytest.raises(TypeError):
        inverse_symmetry(1.0)
    with pytest.raises(TypeError, match="integer tensor"):
        inverse_symmetry(torch.zeros(3))
    g = torch.Generator().manual_seed(3)
    drawn = random_symmetries((64, 5), 5, 6, "cpu", generator=g)
    assert drawn.dtype == torch.uint8 and drawn.shape == (64, 5) and int(drawn.max()) == 3 and int(drawn.min()) == 0
    assert int(random_symmetries((512,), 7, 7, "cpu", generator=g).max()) == 7
    again = random_symmetries((64, 5), 5, 6, "cpu", generator=torch.Generator().manual_seed(3))
    assert torch.equal(drawn, again)
