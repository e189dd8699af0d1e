"""The example learner runs end to end with multi-step targets (--n-step 3), uniform and prioritized."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--prioritized"]])
def test_resident_dqn_example_runs_with_n_step_3(extra):
    spec = importlib.util.spec_from_file_location("train_dqn_resident", os.path.join(ROOT, "examples", "train_dqn_resident.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(["--n-step", "3", "--num-envs", "256", "--board", "8", "--buffer-size", "20000", "--batch-size", "128", "--updates", "6",
                  "--warmup-steps", "4", "--max-steps-per-episode", "30"] + extra)
    assert out["n_step"] == 3 and out["updates"] == 6 and out["ring_fill"] > 0
    assert all(math.isfinite(x) for x in out["loss"]) and len(out["loss"]) >= 1
