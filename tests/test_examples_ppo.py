"""The PPO example runs end to end on the on-device self-play loop (a smoke test: two iterations, finite losses)."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_selfplay_ppo_example_runs():
    spec = importlib.util.spec_from_file_location("train_ppo_selfplay", os.path.join(ROOT, "examples", "train_ppo_selfplay.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    # max_turns below the horizon: every env is truncated and re-dealt inside each rollout, so invalid rows occur
    out = m.main(["--num-envs", "64", "--board", "8", "--players", "2", "--horizon", "16", "--iterations", "2", "--batch-size", "512",
                  "--max-turns", "10"])
    rows = out["iterations"]
    assert len(rows) == 2
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "clip_fraction")), r
        assert 0.0 < r["valid_rows"] < 1.0, r                  # re-deal rows were met (and weighed nothing)
        assert r["entropy"] > 0.0
    assert out["bad_actions"] == 0 and out["rejected"] == 0
    assert out["parameter_change"] > 0.0
