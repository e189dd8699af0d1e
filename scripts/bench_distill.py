#!/usr/bin/env python3
"""The fused policy-distillation loss (MaskedCategoricalHead.distill, gvec_policy_distill / _backward) against the torch
float32 formulation it replaces, in one process, timed with HIP events:

  forward           head.distill (no grad)                | masked_fill -> log_softmax -> (target * logp).sum -> xlogy, entropy sum
  forward+backward  head.distill, grad of the loss        | the same through torch autograd
                    w1 * ce + w2 * kl + w3 * entropy wrt logits
  backward_kernel   gvec_policy_distill_backward called  | -
                    directly on the three weight vectors

The targets are what a search writes: gvec_search_improved_policy on random logits, candidates and playout sums.  The two
sides alternate inside every repeat; a figure is the median over the repeats of the mean time of `iters` calls, and the two
sides' outputs are compared before anything is timed.  `hip_bytes` is the kernels' traffic by construction: 9 A bytes per row
forward (float32 logits, mask bytes, float32 target, each once), 13 A backward (the same and the gradient's store).
forward+backward carries the autograd glue of both sides (the weighted sum, its gradient, a dozen small launches): at the
smaller shape that glue, not the two kernels, sets the fused side's time, which is why the backward kernel is also timed bare.

    python scripts/bench_distill.py [--out profiles/distill_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from generalsreinforcementlearning_amd._lib import PolicyDistillBackwardArgs, SearchPolicyArgs, check, load
from generalsreinforcementlearning_amd.policy_head import MaskedCategoricalHead

SIZES = [(16384, 2000), (8192, 1125)]
SLOTS = 16


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


def search_targets(logits, mask, gen):
    """gvec_search_improved_policy on random search results: SLOTS legal candidates per row, each visited 1 to 4 times with a
    mean score in [-1, 1] (PlayoutScore's default range)."""
    rows, A = logits.shape
    dev = logits.device
    keys = torch.rand(rows, A, device=dev, generator=gen).masked_fill(~mask, -1.0)
    cand = keys.topk(SLOTS, dim=1).indices.contiguous()
    cand = torch.where(mask.gather(1, cand), cand, torch.full_like(cand, -1))        # a row with fewer legal actions: empty slots
    count = torch.randint(1, 5, (rows, SLOTS), device=dev, generator=gen, dtype=torch.int32) * (cand >= 0).int()
    total = (torch.rand(rows, SLOTS, device=dev, generator=gen, dtype=torch.float64) * 2 - 1) * count
    target, v_mix = torch.empty(rows, A, device=dev), torch.empty(rows, device=dev)
    a = SearchPolicyArgs(n=rows, num_actions=A, m=SLOTS, reserved=0, logits=logits.data_ptr(), mask=mask.view(torch.uint8).data_ptr(),
                         candidates0=cand.data_ptr(), sum=total.data_ptr(), count=count.data_ptr(), value=None, q_lo=-1.0,
                         q_inv_range=0.5, c_visit=50.0, c_scale=1.0, target=target.data_ptr(), v_mix=v_mix.data_ptr())
    check(load().gvec_search_improved_policy(dev.index, torch.cuda.current_stream(dev).cuda_stream, C.byref(a)),
          "gvec_search_improved_policy")
    torch.cuda.synchronize()                        # cand, total and count go out of scope below
    return target


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--legal", type=float, default=0.15, help="share of legal actions per row")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py needs a GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    head = MaskedCategoricalHead(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    results = []
    for rows, A in SIZES:
        logits = torch.randn(rows, A, device=dev, generator=gen)
        mask = torch.rand(rows, A, device=dev, generator=gen) < a.legal
        mask[:, 0] = True                           # torch's path turns a row without a legal action into NaN
        target = search_targets(logits, mask, gen)
        w = [torch.randn(rows, device=dev, generator=gen) for _ in range(3)]
        leaf = logits.clone().requires_grad_(True)

        def torch_distill(x=logits):
            lp = torch.log_softmax(x.masked_fill(~mask, float("-inf")), -1)
            lp0 = lp.masked_fill(~mask, 0.0)
            ce = -(target * lp0).sum(-1)
            return ce, torch.xlogy(target, target).sum(-1) + ce, -(lp.exp() * lp0).sum(-1)

        def torch_forward():
            with torch.no_grad():
                return torch_distill()

        def torch_train():
            ce, kl, ent = torch_distill(leaf)
            return torch.autograd.grad((w[0] * ce + w[1] * kl + w[2] * ent).sum(), leaf)[0]

        def hip_forward():
            with torch.no_grad():
                return head.distill(logits, mask, target)

        def hip_train():
            ce, kl, ent = head.distill(leaf, mask, target)
            return torch.autograd.grad((w[0] * ce + w[1] * kl + w[2] * ent).sum(), leaf)[0]

        grad_out = torch.empty_like(logits)
        bw = PolicyDistillBackwardArgs(rows=rows, num_actions=A, logits=logits.data_ptr(), mask=mask.view(torch.uint8).data_ptr(),
                                       target=target.data_ptr(), grad_ce=w[0].data_ptr(), grad_kl=w[1].data_ptr(),
                                       grad_entropy=w[2].data_ptr(), grad_logits=grad_out.data_ptr())
        lib, bw_ref, stream = load(), C.byref(bw), torch.cuda.current_stream(dev).cuda_stream

        def hip_backward_kernel():
            check(lib.gvec_policy_distill_backward(dev.index, stream, bw_ref), "gvec_policy_distill_backward")
            return grad_out

        # the two sides agree before they are timed
        agree = {k: float((x - y).abs().max()) for k, x, y in zip(("ce", "kl", "entropy"), torch_forward(), hip_forward())}
        agree["grad"] = float((torch_train() - hip_train()).abs().max())
        assert torch.equal(hip_backward_kernel(), hip_train())
        moved = {"forward": rows * A * 9 + rows * 12, "forward_backward": rows * A * (9 + 13) + rows * 24, "backward_kernel": rows * A * 13 + rows * 12}
        med = {}
        for name, pair in (("forward", {"hip": hip_forward, "torch": torch_forward}), ("forward_backward", {"hip": hip_train, "torch": torch_train})):
            m, s = timed(pair, a.iters, a.repeats)
            med[name] = {"hip_ms": m["hip"], "torch_ms": m["torch"], "torch_over_hip": m["torch"] / m["hip"],
                         "hip_min_max_ms": s["hip"], "torch_min_max_ms": s["torch"], "hip_bytes": moved[name],
                         "hip_bytes_per_s": moved[name] / (m["hip"] * 1e-3)}
        m, s = timed({"hip": hip_backward_kernel}, a.iters, a.repeats)
        med["backward_kernel"] = {"hip_ms": m["hip"], "hip_min_max_ms": s["hip"], "hip_bytes": moved["backward_kernel"],
                                  "hip_bytes_per_s": moved["backward_kernel"] / (m["hip"] * 1e-3)}
        res = {"rows": rows, "num_actions": A, "legal_share": a.legal, "target_row_sum_min_max": [float(target.sum(1).min()), float(target.sum(1).max())],
               "max_abs_difference_torch_vs_hip": agree, **med}
        print(json.dumps(res))
        results.append(res)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats,
           "note": "median over repeats of the mean ms per call (HIP events), both sides alternating in one process; "
                   "hip_bytes = the kernels' traffic by construction (9 A bytes per row forward, 13 A backward), computed from the shapes; "
                   "forward_backward includes the autograd glue of both sides (the weighted sum and its gradient)", "sizes": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
