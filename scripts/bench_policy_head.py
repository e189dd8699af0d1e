#!/usr/bin/env python3
"""The fused masked-categorical head (MaskedCategoricalHead, gvec_policy_*) against the torch formulation it replaces, in one
process, timed with HIP events:

  sample             head.sample                        | masked_fill -> log_softmax -> Categorical.sample, log_prob, entropy
  evaluate           head.evaluate (no grad)            | masked_fill -> log_softmax -> gather, entropy sum
  evaluate+backward  head.evaluate, grad of the loss    | the same through torch autograd
                     w1 * logp + w2 * entropy wrt logits

The two sides alternate inside every repeat; a figure is the median over the repeats of the mean time of `iters` calls.
`bytes_per_s` of the fused path counts what the algorithm must move: logits + mask read once (twice for evaluate+backward:
each kernel reads them once), grad_logits written once, the per-row vectors.

    python scripts/bench_policy_head.py [--out profiles/policy_head_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from generalsreinforcementlearning_amd.policy_head import MaskedCategoricalHead

SIZES = [(16384, 2000), (8192, 1125)]


def timed(fns, iters, repeats, warmup=3):
    """{name: median ms per call}: warm-up of every fn, then `repeats` rounds that time each fn in turn."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--legal", type=float, default=0.02, help="share of legal actions per row (a real game: about 2 %%)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "policy_head_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_head.py needs a GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    head = MaskedCategoricalHead(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    results = []
    for rows, A in SIZES:
        logits = torch.randn(rows, A, device=dev, generator=gen)
        mask = torch.rand(rows, A, device=dev, generator=gen) < a.legal
        mask[:, 0] = True                           # torch's path turns a row without a legal action into NaN
        actions, _, _ = head.sample(logits, mask, seed=7)
        w1, w2 = torch.randn(rows, device=dev, generator=gen), torch.randn(rows, device=dev, generator=gen)
        leaf = logits.clone().requires_grad_(True)
        seed = [0]

        def torch_logp(x):
            return torch.log_softmax(x.masked_fill(~mask, float("-inf")), -1)

        def torch_sample():
            with torch.no_grad():
                d = torch.distributions.Categorical(logits=torch_logp(logits), validate_args=False)
                act = d.sample()
                return act, d.log_prob(act), d.entropy()

        def torch_evaluate(x=logits):
            lp = torch_logp(x)
            return lp.gather(1, actions[:, None]).squeeze(1), -(lp.exp() * lp.masked_fill(~mask, 0.0)).sum(-1)

        def torch_evaluate_nograd():
            with torch.no_grad():
                return torch_evaluate()

        def torch_train():
            lp, ent = torch_evaluate(leaf)
            return torch.autograd.grad((w1 * lp + w2 * ent).sum(), leaf)[0]

        def hip_sample():
            seed[0] += 1
            return head.sample(logits, mask, seed=seed[0])

        def hip_evaluate():
            with torch.no_grad():
                return head.evaluate(logits, mask, actions)

        def hip_train():
            lp, ent = head.evaluate(leaf, mask, actions)
            return torch.autograd.grad((w1 * lp + w2 * ent).sum(), leaf)[0]

        # the two sides agree before they are timed
        lp_t, ent_t = torch_evaluate_nograd()
        lp_h, ent_h = hip_evaluate()
        agree = {"logp": float((lp_t - lp_h).abs().max()), "entropy": float((ent_t - ent_h).abs().max()),
                 "grad": float((torch_train() - hip_train()).abs().max())}
        row_bytes = rows * A * 5                    # float32 logits + mask bytes, once
        moved = {"sample": row_bytes + rows * 16, "evaluate": row_bytes + rows * 16,
                 "evaluate_backward": 2 * row_bytes + rows * A * 4 + rows * 32}
        med = {}
        for name, pair in (("sample", {"hip": hip_sample, "torch": torch_sample}), ("evaluate", {"hip": hip_evaluate, "torch": torch_evaluate_nograd}),
                           ("evaluate_backward", {"hip": hip_train, "torch": torch_train})):
            m, s = timed(pair, a.iters, a.repeats)
            med[name] = {"hip_ms": m["hip"], "torch_ms": m["torch"], "torch_over_hip": m["torch"] / m["hip"],
                         "hip_min_max_ms": s["hip"], "torch_min_max_ms": s["torch"], "hip_bytes": moved[name],
                         "hip_bytes_per_s": moved[name] / (m["hip"] * 1e-3)}
        res = {"rows": rows, "num_actions": A, "legal_share": a.legal, "max_abs_difference_torch_vs_hip": agree, **med}
        print(json.dumps(res))
        results.append(res)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats, "bad_actions": head.bad_actions,
           "note": "median over repeats of the mean ms per call (HIP events), both sides alternating in one process; "
                   "hip_bytes = the bytes the algorithm must move, computed from the shapes", "sizes": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
