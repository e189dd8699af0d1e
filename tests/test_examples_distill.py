"""The search-distillation example runs end to end (two iterations, finite losses), and the loss it minimises can be
minimised: Adam on distill_loss alone lowers the weighted cross-entropy of one gathered batch."""
import importlib.util
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _example():
    spec = importlib.util.spec_from_file_location("train_search_distill", os.path.join(ROOT, "examples", "train_search_distill.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_search_distill_example_runs(tmp_path, capsys):
    import json
    import torch
    m = _example()
    path = str(tmp_path / "distilled.pt")
    out = m.main(["--num-envs", "16", "--board", "8", "--players", "2", "--horizon", "4", "--iterations", "2", "--batch-size", "64",
                  "--halving", "4:8:4", "--save", path])
    rows = out["iterations"]
    assert len(rows) == 2
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert printed == rows                                      # one line per iteration
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("ce", "kl", "value_loss", "entropy")), r
        assert r["ce"] > 0.0 and r["kl"] >= -1e-6 and r["entropy"] > 0.0 and 0.0 < r["valid_rows"] <= 1.0
    assert out["rejected"] == 0 and out["parameter_change"] > 0.0
    # the checkpoint is one examples/evaluate_arena.py loads, as the PPO example's
    spec = importlib.util.spec_from_file_location("evaluate_arena", os.path.join(ROOT, "examples", "evaluate_arena.py"))
    arena = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(arena)
    net = arena.load_net(path, 8, torch.device("cuda", 0))
    logits, value = net(torch.zeros(3, 9, 8, 8, device="cuda"))
    assert logits.shape == (3, 320) and value.shape == (3,)


def test_adam_on_the_distill_loss_lowers_the_cross_entropy():
    import torch
    import generalsreinforcementlearning_amd as g
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    m = _example()
    torch.manual_seed(0)
    Bn, L, T, side = 16, 2, 4, 8
    N, A = Bn * L, 5 * side * side
    env = GeneralsSelfPlayVecEnv(Bn, side, side, L, max_turns=50, seed=5, board_pool=16, device_outputs=True)
    buf = g.SelfPlayRolloutBuffer(env, T, policy_target=True)
    search = g.HalvingSearch(env, candidates=4, budget=8, depth=4)
    head = g.MaskedCategoricalHead()
    net = m.ActorCritic((9, side, side), A).cuda()
    buf.begin(*env.reset())
    with torch.no_grad():
        while not buf.full:
            logits, value = net(buf.obs.view(N, 9, side, side))
            logits, mask = logits.contiguous(), buf.valid_actions_mask.view(N, A)
            actions, info = search.act(mask, logits, seed=buf._step + 1)
            target, v_mix = search.policy_target(logits, mask, info)
            buf.step(actions, head.evaluate(logits, mask, actions)[0], value, policy_target=target, search_value=v_mix)
        buf.finish(net(buf.obs.view(N, 9, side, side))[1])
    batch = {k: v.clone() for k, v in buf.gather(torch.arange(T * N, device="cuda")).items()}
    assert batch["weight"].sum() > 0
    loss_of = lambda: g.distill_loss(net(batch["obs"])[0], batch["valid_actions_mask"], batch["policy_target"], batch["weight"])
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    with torch.no_grad():
        before = float(loss_of())
    for _ in range(20):
        loss = loss_of()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    with torch.no_grad():
        after = float(loss_of())
    print(f"weighted mean ce before {before:.6f} after 20 Adam steps {after:.6f}")
    assert math.isfinite(before) and math.isfinite(after) and after < before
    env.close()
