"""Scans the gfx950 ISA the build generated (csrc/build/*-gfx950.s, kept by -save-temps) for hazards the compiler
cannot see because they sit inside inline-asm strings.

gfx940 family (gfx950 included): a VMEM store wider than 64 bits needs 2 wait states before a VALU instruction
rewrites its data registers.  Every 16-byte streaming store of the step path goes through `st_through(u32x4*)`
(gvec_device.hpp), an asm string the hazard recognizer does not parse; its trailing `s_nop 1` is the protection
and this test is the proof that no store site lost it."""
import os
import re

import pytest

from generalsreinforcementlearning_amd.csrc import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generalsreinforcementlearning_amd", "csrc")
BUILD = os.path.join(CSRC, "build")
UNITS = [s[:-len(".hip")] for s in B.SRCS]
# the staged 16-byte stores of the whole library, counted on the listing of the build that still had one kernel unit: a scan
# that finds fewer has lost a file
WIDE_STORE_SITES = 1962


def _instructions(path):
    out = []
    for line in open(path):
        s = line.split(";")[0].strip()
        if not s or s.startswith((".", "//")) or s.endswith(":"):
            continue
        out.append(s)
    return out


def _wide_store_sites(unit):
    """(instructions, indices of the 16-byte streaming stores) of one unit's listing"""
    path = os.path.join(BUILD, f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(path):
        B.build(force=True, verbose=False)
    ins = _instructions(path)
    return ins, [i for i, s in enumerate(ins) if re.match(r"global_store_dwordx[34]\b.*\bsc1\b", s)]


@pytest.mark.parametrize("unit", UNITS)
def test_wide_asm_stores_keep_their_wait_states(unit):
    ins, sites = _wide_store_sites(unit)
    if unit in ("gvec_kernels", "gvec_gym"):
        assert len(sites) > 100, "the step path's staged 16-byte stores were not found: has st_through changed its spelling?"
    for i in sites:
        nxt = ins[i + 1]
        m = re.match(r"s_nop\s+(\d+)", nxt)
        if m and int(m.group(1)) >= 1:
            continue
        # without the nop: the next two instructions must not be VALU writes of the store's data registers
        regs = re.search(r"v\[(\d+):(\d+)\]", ins[i].split(",")[1])
        lo, hi = int(regs.group(1)), int(regs.group(2))
        for k in (1, 2):
            dst = re.match(r"v_\w+\s+v(?:\[(\d+):(\d+)\]|(\d+))", ins[i + k])
            if dst:
                a = int(dst.group(1) or dst.group(3))
                b = int(dst.group(2) or dst.group(3))
                assert b < lo or a > hi, f"{unit}: `{ins[i]}` is followed within 2 wait states by `{ins[i + k]}`"


def test_wide_store_scan_covers_every_unit():
    assert sum(len(_wide_store_sites(unit)[1]) for unit in UNITS) >= WIDE_STORE_SITES


def test_every_source_is_built_and_watched():
    """A unit left out of SRCS is missing from the library, a header left out of DEPS from the rebuild check."""
    names = sorted(os.listdir(CSRC))
    assert sorted(n for n in names if n.endswith(".hip")) == sorted(B.SRCS)
    assert {n for n in names if n.endswith(".hpp")} <= set(B.DEPS)
    # build.py watches a HOST_DEPS header for the gvec_api* units alone: no other unit or header may include one
    for n in names:
        if n.endswith((".hip", ".hpp", ".inc")) and not n.startswith("gvec_api") and n not in B.HOST_DEPS:
            text = open(os.path.join(CSRC, n)).read()
            assert not [d for d in B.HOST_DEPS if f'"{d}"' in text], n


def test_no_cross_lane_read_behind_a_short_circuit():
    """ds_bpermute / DPP read zeros from lanes that are masked off in EXEC.  A `cond && gather(...)` whose `cond` differs
    between lanes evaluates the gather for some lanes only - and the others' bits vanish from what the active lanes read (the
    first aligned-window version of gym_emit lost its type planes that way).  The kernels' idiom is: cross-lane reads into
    locals first, then the logic; this scan keeps it that way."""
    import re
    src_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generalsreinforcementlearning_amd", "csrc")
    pat = re.compile(r"(&&|\|\||\?)\s*!?\s*(at|arm_at|bperm|rdlane_any|b\.gather|b\.gather_mask|gather|gather_mask)\s*\(")
    bad = []
    for name in sorted(os.listdir(src_dir)):
        if name.endswith((".hip", ".hpp")):
            for i, line in enumerate(open(os.path.join(src_dir, name)), 1):
                code = line.split("//")[0]
                if pat.search(code):
                    bad.append(f"{name}:{i}: {line.strip()}")
    assert not bad, "\n".join(bad)
