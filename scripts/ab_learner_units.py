#!/usr/bin/env python3
"""The subsystems' own bench scripts against two builds of the library in ONE process, in the order BASE, NEW, BASE: each
script runs three times at its default sizes with GVEC_LIB naming the build (generalsreinforcementlearning_amd._lib.load
honours it), and the gap between the two BASE runs is the noise the NEW run is judged by.  Per timing the script reports
(a numeric leaf of its JSON line whose key says us or ms): [base, new, base again] and `inside` = new <= the slower base run
+ |base - base again|.  Writes one JSON document.

usage: scripts/ab_learner_units.py BASE.so NEW.so [--out profiles/learner_units_ab.json] [--only rollout,nstep,...]"""
import argparse
import contextlib
import gc
import io
import json
import os
import re
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

from generalsreinforcementlearning_amd import _lib  # noqa: E402

# script -> its arguments: default sizes; the torch baselines and the end-to-end parts that run no kernel under test are skipped
SCRIPTS = {"rollout": ["--out", os.devnull], "nstep": ["--out", os.devnull], "pool": [], "features": ["--skip-torch"],
           "memory": ["--skip-torch", "--skip-rollout"], "qtarget": [], "per": ["--out", os.devnull], "stream_deltas": []}

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "learner_units_ab.json"))
ap.add_argument("--only", default="rollout,nstep,pool,features,memory,qtarget")
args = ap.parse_args()
BASE, NEW = (os.path.abspath(p) for p in args.libs)


def run(name, lib):
    """the JSON line `scripts/bench_<name>.py` prints with `lib` loaded"""
    os.environ["GVEC_LIB"], _lib._LIB = lib, None
    argv, sys.argv = sys.argv, [os.path.join(HERE, f"bench_{name}.py")] + SCRIPTS[name]
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        sys.argv = argv
    print(f"bench_{name}.py with {lib}: done", file=sys.stderr, flush=True)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return json.loads([line for line in text.getvalue().splitlines() if line.startswith("{")][-1])


def timings(doc, path=""):
    """{path: value} of the numeric leaves whose key names a time"""
    out = {}
    items = doc.items() if isinstance(doc, dict) else enumerate(doc) if isinstance(doc, list) else ()
    for k, v in items:
        p = f"{path}/{k}"
        if isinstance(v, (dict, list)):
            out.update(timings(v, p))
        elif isinstance(v, (int, float)) and not isinstance(v, bool) and re.search(r"(^|_)(us|ms)(_|$)", str(k)):
            out[p] = float(v)
    return out


result = {"bench": "ab_learner_units", "device": torch.cuda.get_device_name(0), "order": ["base", "new", "base_again"], "scripts": {}}
for name in args.only.split(","):
    a, b, c = (timings(run(name, lib)) for lib in (BASE, NEW, BASE))
    rows = {}
    for key in a:
        if key in b and key in c:
            rows[key] = {"base": a[key], "new": b[key], "base_again": c[key], "inside": bool(b[key] <= max(a[key], c[key]) + abs(a[key] - c[key]))}
    result["scripts"][f"bench_{name}.py"] = rows
    print(name, sum(r["inside"] for r in rows.values()), "of", len(rows), "timings inside", file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
