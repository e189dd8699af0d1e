"""The PPO example with --features: the torso takes 9 + 5 channels, the five strategic feature planes recomputed from the
stored nine-plane observations while acting and on every minibatch (a smoke test: one iteration, finite losses)."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_selfplay_ppo_example_runs_with_features():
    spec = importlib.util.spec_from_file_location("train_ppo_selfplay", os.path.join(ROOT, "examples", "train_ppo_selfplay.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(["--features", "--iterations", "1", "--num-envs", "64", "--board", "8", "--horizon", "8"])
    rows = out["iterations"]
    assert len(rows) == 1
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "clip_fraction")), r
    assert out["bad_actions"] == 0 and out["rejected"] == 0
    assert out["parameter_change"] > 0.0
