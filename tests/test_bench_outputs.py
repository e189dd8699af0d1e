"""bench.py's plain line, --full and --dump-outputs: a plain run times its steps and nothing else, the extra figures come
with --full, and the dumped outputs of the last timed step are the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "7", "--warmup", "3", "--prewarm-steps", "40", "--envs-per-gpu", "1500", "--pool", "64",
         "--width", "12", "--height", "12", "--players", "3"]


def _plain_env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=_plain_env())
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_bench_refuses_a_run_without_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=_plain_env())
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumped_outputs_repeat_and_full_adds_only_figures(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    f = _bench("--dump-outputs", str(tmp_path / "f"), "--full", "--no-cpu-baseline")
    for d in (a, b):
        assert d["steps"] == 7 and d["warmup"] == 3 and d["prewarm_steps"] == 40 and d["ms_per_step"] > 0
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
        assert "fused_rollout" not in d and "cpu_baseline" not in d
    assert f["fused_rollout"]["env_steps_per_s_per_gpu"] > 0
    for k in ("env_steps_played", "aborted_turns", "games_finished"):
        assert a[k] == b[k] == f[k], k
    oa, ob, of = _load(tmp_path / "a"), _load(tmp_path / "b"), _load(tmp_path / "f")
    assert {"army", "owner", "turn", "done", "army_count", "legal_mask_bits", "env_index"} <= set(oa)
    assert sum(x.nbytes for x in oa.values()) <= 64 << 20
    n = len(oa["env_index"])
    assert n == 1500 and (np.diff(oa["env_index"]) > 0).all()   # 1,500 boards fit the sample: all of them, in order
    for name, x in oa.items():
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == n, name
        np.testing.assert_array_equal(x, ob[name], err_msg=name)
        np.testing.assert_array_equal(x, of[name], err_msg=name)   # written before --full's fused rollout steps the boards
    assert oa["army"].dtype == np.float64 and oa["legal_mask_bits"].max() <= 255 and oa["legal_mask_bits"].any()
