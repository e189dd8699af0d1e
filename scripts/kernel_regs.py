#!/usr/bin/env python3
"""Register / scratch / LDS use of every kernel variant matching a pattern, read from the gfx950 listings csrc/build.py keeps
for every unit (csrc/build/*-gfx950.s; run the build first).
usage: scripts/kernel_regs.py [substring, default Li4ELi7]"""
import glob, os, re, sys
pat = sys.argv[1] if len(sys.argv) > 1 else "Li4ELi7"
build = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "generalsreinforcementlearning_amd", "csrc", "build")
listings = sorted(glob.glob(os.path.join(build, "*-gfx950.s")))
if not listings:
    sys.exit(f"no listings in {build}: run generalsreinforcementlearning_amd/csrc/build.py first")
for path in listings:
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(path).read(), re.S):
        if pat not in m.group(1):
            continue
        g = lambda k: re.search(r"\.amdhsa_" + k + r"\s+(\S+)", m.group(2)).group(1)
        print(f"{m.group(1)[:64]:64s} vgpr {g('next_free_vgpr'):>4s} sgpr {g('next_free_sgpr'):>4s} scratch {g('private_segment_fixed_size'):>5s} lds {g('group_segment_fixed_size'):>5s}")
