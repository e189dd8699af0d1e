"""The example learner runs end to end with --augment (a board symmetry per sampled row, symmetry.py): on the plain
sampling path, and with categorical targets over prioritized n-step replay.  The flag adds one key to the result."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--num-envs", "256", "--board", "8", "--buffer-size", "20000", "--batch-size", "128", "--updates", "6", "--warmup-steps", "4",
          "--max-steps-per-episode", "30"]
TODAY = ["env_steps", "env_steps_per_s", "episodes", "loss", "mean_episode_reward", "n_step", "ring_fill", "seconds", "updates",
         "updates_per_s"]


def _example():
    spec = importlib.util.spec_from_file_location("train_dqn_resident", os.path.join(ROOT, "examples", "train_dqn_resident.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("extra,more_keys", [([], []), (["--categorical", "--prioritized", "--n-step", "3"], ["targets"])],
                         ids=["alone", "categorical_prioritized_nstep"])
def test_resident_dqn_example_runs_with_augment(extra, more_keys):
    out = _example().main(COMMON + ["--augment"] + extra)
    assert out["augment"] is True and out["updates"] == 6 and out["ring_fill"] > 0
    assert all(math.isfinite(x) for x in out["loss"]) and len(out["loss"]) >= 1
    assert sorted(out) == sorted(TODAY + ["augment"] + more_keys)
