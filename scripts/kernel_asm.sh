#!/bin/bash
# Dumps the ISA of one kernel (default: the headline step kernel) to k.s in the current directory, comments stripped, from
# the gfx950 listings csrc/build.py keeps for every unit (run the build first).
K=${1:-_ZN4gvec11step_kernelILi4ELi7ELb1ELb1EEEvNS_8StepArgsE}
BUILD="$(cd "$(dirname "$0")/../generalsreinforcementlearning_amd/csrc/build" && pwd)" || exit 1
cat "$BUILD"/*-gfx950.s | awk "/^$K:/,/\.Lfunc_end/" | grep -v "^\s*;\|\.loc\|Ltmp\|implicit-def" > k.s
wc -l k.s
