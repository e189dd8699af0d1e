"""The PPO example with --memory: the torso takes 9 + 4 channels, the four fog-of-war memory planes stored per step beside the
observations; with --features as well 9 + 4 + 5, the features computed from the remembered observation (a smoke test: one
iteration, finite losses)."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("flags,channels", [(["--memory"], 13), (["--memory", "--features"], 18)], ids=["memory", "memory_features"])
def test_selfplay_ppo_example_runs_with_memory(flags, channels, monkeypatch):
    spec = importlib.util.spec_from_file_location("train_ppo_selfplay", os.path.join(ROOT, "examples", "train_ppo_selfplay.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    seen = []
    net = m.ActorCritic

    def counting(obs_shape, n_actions, **kw):
        seen.append(obs_shape[0])
        return net(obs_shape, n_actions, **kw)

    monkeypatch.setattr(m, "ActorCritic", counting)
    out = m.main(flags + ["--iterations", "1", "--num-envs", "64", "--board", "8", "--horizon", "8"])
    assert seen == [channels]
    rows = out["iterations"]
    assert len(rows) == 1
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "clip_fraction")), r
    assert out["bad_actions"] == 0 and out["rejected"] == 0
    assert out["parameter_change"] > 0.0
