#!/usr/bin/env python3
"""V-trace targets (gvec_traj_vtrace) against the same definition as a Python loop of T torch steps, with gvec_traj_gae on the
same flags next to it, in one process, alternating and repeated; writes profiles/vtrace_bench.json and prints the same JSON
line.  T = 128, N = 8,192 / 131,072 / 1,048,576 streams.
  bytes per row, by construction: GAE reads reward 8 + value 4 + flags 1 and writes adv 4 + ret 4 = 21; V-trace reads the two
  log-probs as well and writes rho: 21 + 8 + 4 = 33 (29 with rho_out = NULL).
Times are host clocks around work that ends in a device synchronise.
usage: scripts/bench_vtrace.py [--streams N,N,...] [--horizon T] [--repeats R] [--iters K]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import generalsreinforcementlearning_amd as g
from generalsreinforcementlearning_amd._lib import TrajGaeArgs, TrajVtraceArgs, check

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="8192,131072,1048576")
ap.add_argument("--horizon", type=int, default=128)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vtrace_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
GAMMA, LAM, RHO_BAR, C_BAR = 0.99, 0.95, 1.0, 1.0


def timed(fns, iters, repeats):
    """Median wall ms per call of each function, the functions alternating inside every repeat."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e3)
    return {k: {"ms": round(sorted(v)[len(v) // 2], 5), "ms_all": [round(x, 5) for x in v]} for k, v in times.items()}


def torch_vtrace(reward, value, flags, lt, lb, vs, pg, rho_out):
    T = reward.shape[0]
    v = value.double()
    valid, terminal, cut = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
    w = torch.exp(lt.double() - lb.double())
    rho, glc = w.clamp(max=RHO_BAR), GAMMA * LAM * w.clamp(max=C_BAR)
    acc, vs_next = torch.zeros_like(reward[0]), v[T]
    for t in range(T - 1, -1, -1):
        nv = torch.where(terminal[t], 0.0, v[t + 1])
        nvs = torch.where(terminal[t], 0.0, torch.where(cut[t], v[t + 1], vs_next))
        delta = rho[t] * ((reward[t] + GAMMA * nv) - v[t])
        acc = torch.where(valid[t], delta + glc[t] * torch.where(cut[t], 0.0, acc), 0.0)
        vs_next = v[t] + acc
        vs[t] = vs_next
        pg[t] = torch.where(valid[t], rho[t] * ((reward[t] + GAMMA * nvs) - v[t]), 0.0)
        rho_out[t] = torch.where(valid[t], rho[t], 0.0)
    x, r = pg[valid].double(), rho_out[valid].double()
    return torch.stack([valid.sum().double(), x.sum(), (x * x).sum(), r.sum()])


def bench(N, T):
    L = g.load()
    gen = torch.Generator(device=dev)
    gen.manual_seed(N)
    reward = torch.randn(T, N, dtype=torch.float64, device=dev, generator=gen)
    value = torch.randn(T + 1, N, device=dev, generator=gen)
    u = torch.rand(T, N, device=dev, generator=gen)
    flags = torch.where(u < 0.02, 0, torch.where(u < 0.04, 7, torch.where(u < 0.06, 5, 1))).to(torch.uint8)
    lb = -3.0 * torch.rand(T, N, device=dev, generator=gen)
    lt = lb + 0.5 * torch.randn(T, N, device=dev, generator=gen)
    z = lambda: torch.zeros(T, N, device=dev)
    vs, pg, rho, adv, ret, vs2, pg2, rho2 = (z() for _ in range(8))
    stats, gae_stats = (torch.zeros(4, dtype=torch.float64, device=dev) for _ in range(2))
    scratch = torch.zeros(int(L.gvec_traj_scratch_bytes(T, N)), dtype=torch.uint8, device=dev)
    va = TrajVtraceArgs(T=T, N=N, gamma=GAMMA, lam=LAM, rho_bar=RHO_BAR, c_bar=C_BAR, reward=reward.data_ptr(), value=value.data_ptr(),
                        flags=flags.data_ptr(), logp_behaviour=lb.data_ptr(), logp_target=lt.data_ptr(), vs=vs.data_ptr(), pg=pg.data_ptr(),
                        rho_out=rho.data_ptr(), stats=stats.data_ptr(), scratch=scratch.data_ptr())
    ga = TrajGaeArgs(T=T, N=N, gamma=GAMMA, lam=LAM, reward=reward.data_ptr(), value=value.data_ptr(), flags=flags.data_ptr(),
                     adv=adv.data_ptr(), ret=ret.data_ptr(), stats=gae_stats.data_ptr(), scratch=scratch.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    r = timed({"vtrace_hip": lambda: check(L.gvec_traj_vtrace(0, stream, C.byref(va)), "gvec_traj_vtrace"),
               "gae_hip": lambda: check(L.gvec_traj_gae(0, stream, C.byref(ga)), "gvec_traj_gae"),
               "vtrace_torch_loop": lambda: torch_vtrace(reward, value, flags, lt, lb, vs2, pg2, rho2)}, args.iters, args.repeats)
    check(L.gvec_traj_vtrace(0, stream, C.byref(va)), "gvec_traj_vtrace")
    want = torch_vtrace(reward, value, flags, lt, lb, vs2, pg2, rho2)
    torch.cuda.synchronize()
    vb, gb = T * N * 33, T * N * 21
    r.update({"streams": N, "horizon": T, "vtrace_bytes": vb, "gae_bytes": gb,
              "max_abs_diff_vs": float((vs - vs2).abs().max()), "max_abs_diff_pg": float((pg - pg2).abs().max()),
              "max_abs_diff_rho": float((rho - rho2).abs().max()), "mean_rho": float(stats[3] / stats[0]),
              "stats_rel_diff": float(((stats - want).abs() / want.abs().clamp_min(1.0)).max()),
              "vtrace_GBps": round(vb / r["vtrace_hip"]["ms"] / 1e6, 1), "gae_GBps": round(gb / r["gae_hip"]["ms"] / 1e6, 1),
              "vtrace_over_gae": round(r["vtrace_hip"]["ms"] / r["gae_hip"]["ms"], 3),
              "speedup_over_torch_loop": round(r["vtrace_torch_loop"]["ms"] / r["vtrace_hip"]["ms"], 2)})
    return r


rows = []
for n in args.streams.split(","):
    rows.append(bench(int(n), args.horizon))
    torch.cuda.empty_cache()
result = {"bench": "vtrace", "repeats": args.repeats, "iters": args.iters, "gamma": GAMMA, "lambda": LAM, "rho_bar": RHO_BAR,
          "c_bar": C_BAR, "rows": rows}
line = json.dumps(result)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1) + "\n")
print(line)
