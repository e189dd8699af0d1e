#!/usr/bin/env python3
"""Compares two builds' gfx950 ISA listings kernel symbol by kernel symbol: did a source change alter the generated code?

usage: scripts/isa_diff.py OLD NEW [--quiet]
OLD and NEW each name one build: a listing, several joined by commas, or a directory of them (csrc/build: every *-gfx950.s).
The kernels of a build are those of all its listings; a symbol that two listings of one build define is an error.

A kernel's instructions are normalised the way bench.py's step_kernel_isa_hash does it (directives, comments and labels
dropped, the function's index stripped from .LBB labels), so a kernel that merely moved inside the file reports `same`.
Every kernel prints `same` or `differs` (with --quiet: only the differing ones); a differing one also prints the old and new
resource fields.  Last lines: the counts per kernel template.  Exit status 1 when a symbol exists in one listing only."""
import collections
import glob
import hashlib
import os
import re
import sys

FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size", "; Occupancy", "; codeLenInByte")


def kernels(path):
    """{symbol: (sha256 of the normalised instructions, {field: value})} of every .amdhsa_kernel of the listing"""
    out, sym, hh, fields, tail = {}, None, None, None, False
    start = re.compile(r"^(\w+):\s*(;.*)?$")
    for line in open(path):
        if sym is None:
            m = start.match(line)
            if m and not m.group(1).startswith(".L"):
                sym, hh, fields, tail = m.group(1), hashlib.sha256(), {}, False
            continue
        s = line.strip()
        for f in FIELDS:
            if s.startswith(f):
                fields[f] = re.sub(r"^[:=\s]+", "", s[len(f):])
        if s.startswith(".Lfunc_end"):
            tail = True
        elif tail and s.startswith("; Occupancy"):   # the last field of the "Kernel info" comment block
            if ".amdhsa_next_free_vgpr" in fields:   # device functions have no kernel descriptor
                out[sym] = (hh.hexdigest(), fields)
            sym = None
        elif not tail:
            t = line.split(";")[0].strip()
            if t and not t.startswith((".", "//")) and not re.match(r"^\.?L[A-Za-z_0-9]*:$", t):
                hh.update(re.sub(r"\.LBB\d+_", ".LBB_", t).encode() + b"\n")
    return out


def build_kernels(spec):
    """kernels() of every listing of one build"""
    out = {}
    for item in spec.split(","):
        for path in sorted(glob.glob(os.path.join(item, "*-gfx950.s"))) if os.path.isdir(item) else [item]:
            found = kernels(path)
            twice = sorted(set(found) & set(out))
            if twice:
                sys.exit(f"{path}: {len(twice)} kernel symbol(s) already defined by another listing of {spec}, e.g. {twice[0]}")
            out.update(found)
    return out


def template_of(sym):
    m = re.match(r"_ZN(\d+)", sym)   # _ZN4gvec15gym_step_kernelILi2E... -> gym_step_kernel
    n = m and re.match(r"\d+", sym[m.end() + int(m.group(1)):])
    if not n:
        return sym
    at = m.end() + int(m.group(1)) + n.end()
    return sym[at:at + int(n.group(0))]


def main():
    args = [a for a in sys.argv[1:] if a != "--quiet"]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = build_kernels(args[0]), build_kernels(args[1])
    quiet, tally = "--quiet" in sys.argv, collections.defaultdict(lambda: [0, 0])
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            print(f"{sym} only in {'NEW' if sym in new else 'OLD'}")
            continue
        same = old[sym][0] == new[sym][0]
        tally[template_of(sym)][0 if same else 1] += 1
        if not same or not quiet:
            print(f"{sym} {'same' if same else 'differs'}")
        if not same:
            for f in FIELDS:
                print(f"    {f.lstrip('.; '):36s} {old[sym][1].get(f, '?'):>8s} -> {new[sym][1].get(f, '?'):>8s}")
    for t, (s, d) in sorted(tally.items()):
        print(f"{t}: {s} same, {d} differ")
    sys.exit(1 if set(old) != set(new) else 0)


if __name__ == "__main__":
    main()
