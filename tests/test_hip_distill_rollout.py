"""SelfPlayRolloutBuffer(policy_target=True) on the GPU: the target and search-value stores, `policy_target_slot`, what `gather`
returns, a twin buffer without the option, and the loop search -> target -> step -> distill end to end.
An 8x8 board, 2 players, 8 envs, horizon 4 throughout."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, L, T, SIDE = 8, 2, 4, 8
N, A = B * L, 5 * SIDE * SIDE


def _env(seed=3, max_turns=3):
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    return GeneralsSelfPlayVecEnv(B, SIDE, SIDE, L, max_turns=max_turns, seed=seed, board_pool=16, device_outputs=True)


def _actions_from_mask(mask, gen):
    import torch
    m = mask.reshape(N, A).float()
    m[:, 0] += (m.sum(1) == 0).float()
    return torch.multinomial(m, 1, generator=gen).reshape(B, L)


def _rollout(buf, env, seed, through_slot=False, with_target=True):
    """One full rollout on seeded draws; the targets are random rows (the store does not care what they mean)."""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    buf.begin(*env.reset())
    given = []
    while not buf.full:
        a = _actions_from_mask(buf.valid_actions_mask, gen)
        logp, value = torch.randn(B, L, device="cuda", generator=gen), torch.randn(B, L, device="cuda", generator=gen)
        target, sv = torch.rand(B, L, A, device="cuda", generator=gen), torch.randn(B, L, device="cuda", generator=gen)
        given.append((target, sv))
        if not with_target:
            buf.step(a, logp, value)
        elif through_slot:
            slot = buf.policy_target_slot
            assert slot.shape == (B, L, A) and slot.data_ptr() == buf.target_store[len(given) - 1].data_ptr()
            slot.copy_(target)
            buf.step(a, logp, value, policy_target=slot, search_value=sv)
        else:
            buf.step(a, logp, value, policy_target=target, search_value=sv)
    buf.finish(torch.randn(B, L, device="cuda", generator=gen))
    return given


def test_stored_targets_come_back_from_gather():
    import torch
    import generalsreinforcementlearning_amd as g
    env = _env()
    buf = g.SelfPlayRolloutBuffer(env, T, policy_target=True)
    assert buf.target_store.shape == (T, N, A) and buf.target_store.dtype == torch.float32 and not buf.target_store.any()
    assert buf.search_value_store.shape == (T, N) and buf.search_value_store.dtype == torch.float32 and not buf.search_value_store.any()
    given = _rollout(buf, env, 21)
    with pytest.raises(RuntimeError):
        buf.policy_target_slot                                 # the rollout is full: there is no slot T
    for k, (target, sv) in enumerate(given):
        assert torch.equal(buf.target_store[k], target.view(N, A)) and torch.equal(buf.search_value_store[k], sv.view(N))
    rows, values = buf.target_store.view(T * N, A), buf.search_value_store.view(T * N)
    every = torch.arange(T * N, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    shuffled = torch.randperm(T * N, device="cuda", generator=gen)[:37]
    for pos in (every, shuffled):
        batch = buf.gather(pos)
        assert batch["policy_target"].shape == (pos.numel(), A) and batch["policy_target"].dtype == torch.float32
        assert torch.equal(batch["policy_target"], rows[pos]) and torch.equal(batch["search_value"], values[pos])
        assert torch.equal(batch["weight"], buf.valid.reshape(-1)[pos].float())
    assert not buf.valid.all() and buf.valid.any()             # max_turns below the horizon: re-deal rows were met
    seen = torch.cat([b["index"] for b in buf.minibatches(24, seed=1)])
    assert torch.equal(seen.sort().values, every)
    for b in buf.minibatches(24, seed=1):
        assert torch.equal(b["policy_target"], rows[b["index"]]) and torch.equal(b["search_value"], values[b["index"]])
    # positions outside the rollout: counted, weight 0, the nearest row's target
    out = buf.gather(torch.tensor([-3, T * N, 5], device="cuda"))
    assert out["weight"][:2].tolist() == [0.0, 0.0] and int(buf.rejected.item()) == 2
    assert torch.equal(out["policy_target"], rows[torch.tensor([0, T * N - 1, 5], device="cuda")])
    # a step without its search value stores zeros; the next rollout overwrites the rows
    buf.next_rollout()
    buf.step(torch.zeros(B, L, dtype=torch.int64, device="cuda"), torch.zeros(B, L, device="cuda"), torch.zeros(B, L, device="cuda"),
             policy_target=torch.full((B, L, A), 0.25, device="cuda"))
    assert (buf.target_store[0] == 0.25).all() and not buf.search_value_store[0].any()
    assert torch.equal(buf.target_store[1], given[1][0].view(N, A))
    with pytest.raises(ValueError):
        buf.step(torch.zeros(B, L, dtype=torch.int64, device="cuda"), torch.zeros(B, L, device="cuda"), torch.zeros(B, L, device="cuda"))
    env.close()


def test_writing_through_the_slot_equals_passing_a_tensor():
    import torch
    import generalsreinforcementlearning_amd as g
    stores = []
    for through_slot in (False, True):
        env = _env()
        buf = g.SelfPlayRolloutBuffer(env, T, policy_target=True)
        _rollout(buf, env, 21, through_slot=through_slot)
        stores.append((buf.target_store.clone(), buf.search_value_store.clone(), buf.action.clone(), buf.flags.clone()))
        env.close()
    for x, y in zip(*stores):
        assert torch.equal(x, y)
    assert stores[0][0].any()


def test_a_buffer_without_the_option_is_unchanged():
    import torch
    import generalsreinforcementlearning_amd as g
    batches = []
    for with_target in (True, False):
        env = _env()
        buf = g.SelfPlayRolloutBuffer(env, T, policy_target=with_target)
        _rollout(buf, env, 21, with_target=with_target)
        keep = lambda b: {k: v.clone() for k, v in b.items()}  # a gather reuses the tensors of the last one of its size
        batches.append([keep(buf.gather(torch.arange(T * N, device="cuda")))] + [keep(b) for b in buf.minibatches(24, epochs=2, seed=8)])
        if not with_target:
            assert buf.target_store is None and buf.search_value_store is None and buf.policy_target_slot is None
            with pytest.raises(ValueError):
                buf.step(torch.zeros(B, L, dtype=torch.int64, device="cuda"), torch.zeros(B, L, device="cuda"),
                         torch.zeros(B, L, device="cuda"), policy_target=torch.zeros(B, L, A, device="cuda"))
        env.close()
    plain_keys = {"obs", "valid_actions_mask", "action", "logp", "value", "returns", "advantages", "weight", "index"}
    assert len(batches[0]) == len(batches[1])
    for full, plain in zip(*batches):
        assert set(plain) == plain_keys and set(full) == plain_keys | {"policy_target", "search_value"}
        for k in plain_keys:
            assert torch.equal(full[k], plain[k]), k


def test_search_target_step_distill_end_to_end():
    import torch
    import generalsreinforcementlearning_amd as g
    env = _env(max_turns=50)
    buf = g.SelfPlayRolloutBuffer(env, T, policy_target=True)
    search = g.HalvingSearch(env, candidates=4, budget=8, depth=4)
    head = g.MaskedCategoricalHead()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    buf.begin(*env.reset())
    acted = []
    while not buf.full:
        logits = torch.randn(N, A, device="cuda", generator=gen)
        mask = buf.valid_actions_mask.view(N, A)
        actions, info = search.act(mask, logits, seed=100 + len(acted))
        target, v_mix = search.policy_target(logits, mask, info, value=None)
        if len(acted) % 2:                                     # every other step: the search writes the slot itself
            slot = buf.policy_target_slot
            into, v_again = search.policy_target(logits, mask, info, value=None, out=slot.view(N, A))
            assert into.data_ptr() == slot.data_ptr() and torch.equal(into, target) and torch.equal(v_again, v_mix)
            target = slot
        logp, _ = head.evaluate(logits, mask, actions)
        acted.append((logits, mask.clone(), target.clone().view(N, A)))
        buf.step(actions, logp, torch.zeros(N, device="cuda"), policy_target=target, search_value=v_mix)
    buf.finish(torch.zeros(B, L, device="cuda"))
    logits, mask = torch.stack([x for x, _, _ in acted]), torch.stack([m for _, m, _ in acted])    # [T, N, A]
    assert torch.equal(buf.target_store, torch.stack([t for _, _, t in acted]))
    live = mask.any(-1)
    sums = buf.target_store.sum(-1)
    assert live.any() and (sums[live] - 1).abs().max() < 1e-5 and (sums[~live] == 0).all()
    assert (buf.target_store[~mask] == 0).all() and torch.isfinite(buf.search_value_store).all()
    ce, kl, ent = head.distill(logits, mask, buf.target_store)
    assert ce.shape == (T, N) and torch.isfinite(ce).all() and torch.isfinite(kl).all()
    print(f"kl of the acting logits against the search target: min {float(kl.min()):.3e} mean {float(kl.mean()):.3e}")
    assert (kl >= -1e-6).all() and kl.max() > 0
    batch = buf.gather(torch.arange(T * N, device="cuda"))
    assert torch.equal(head.distill(logits.view(T * N, A), batch["valid_actions_mask"], batch["policy_target"])[1], kl.view(-1))
    env.close()
