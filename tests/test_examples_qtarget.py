"""The example learner runs end to end with the masked targets: masked Double DQN, and categorical (C51) with uniform and
with prioritized n-step replay.  Without any of the flags its result has the keys it always had."""
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
@pytest.mark.parametrize("extra,targets", [(["--masked-targets", "--double"], "double"), (["--categorical", "--atoms", "51"], "categorical51"),
                                           (["--categorical", "--prioritized", "--n-step", "3"], "categorical51")],
                         ids=["masked_double", "categorical", "categorical_prioritized_nstep"])
def test_resident_dqn_example_runs_with_masked_targets(extra, targets):
    out = _example().main(COMMON + extra)
    assert out["targets"] == targets and out["updates"] == 6 and out["ring_fill"] > 0
    assert all(math.isfinite(x) for x in out["loss"]) and len(out["loss"]) >= 1
    assert sorted(out) == sorted(TODAY + ["targets"])


@pytest.mark.gpu
def test_without_the_flags_the_result_has_the_keys_it_always_had():
    out = _example().main(COMMON)
    assert sorted(out) == TODAY and out["ring_fill"] > 0 and all(math.isfinite(x) for x in out["loss"])
