#!/usr/bin/env python3
"""Prioritized replay on the device ring (gvec_per_*): the cost of a draw, an update and a push over ring
sizes and batch sizes, against the uniform draw and a torch pow + cumsum + searchsorted route, and the resident pool's
transitions/s with the prioritized ring against the uniform one.  One process, every shape warmed up, medians of event
timings.  Writes profiles/per_bench.json and prints it as one JSON line.

    scripts/bench_per.py [--out profiles/per_bench.json] [--no-pool] [--reps 30]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_per.py --no-pool --reps 5`."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from generalsreinforcementlearning_amd.env_pool import ParallelVecEnvPool
from generalsreinforcementlearning_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_bench.json"))
ap.add_argument("--no-pool", action="store_true")
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda", 0)
COPY_FLOOR_TBPS = 6.29                      # the device-to-device copy rate


def timed(fn, reps=a.reps, warm=5, inner=10):
    """Median over `reps` of the event time of `inner` calls, in microseconds per call."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(out)


def torch_route(pri, size, k, beta, gen):
    """What a learner would write with torch alone: float32 cumsum over the whole ring, searchsorted, weights."""
    c = torch.cumsum(pri, 0)
    total = c[-1]
    t = (torch.arange(k, device=dev) + torch.rand(k, device=dev, generator=gen)) / k * total
    idx = torch.searchsorted(c, t, right=True).clamp_(max=pri.numel() - 1)
    w = (size * pri[idx] / total) ** -beta
    return idx, w / w.max()


out = {"device": torch.cuda.get_device_name(0), "copy_floor_TBps": COPY_FLOOR_TBPS, "sample": [], "update": [], "push": []}
gen = torch.Generator(device=dev)
for cap in (1 << 16, 1 << 20, 1 << 24):
    buf = PrioritizedDeviceReplayBuffer(cap, alpha=0.6, beta=0.4).allocate((1,))
    size = cap * 3 // 4                                            # a quarter of the ring never written: leaves 0
    buf.counters[:3] = torch.tensor([size, size, size])
    td = torch.rand(size, device=dev, generator=gen) * 3
    buf.update_priorities(torch.arange(size, device=dev), td)
    pri = buf.tree[buf.tree_offsets[0]:buf.tree_offsets[0] + cap]
    uni = DeviceReplayBuffer(cap).allocate((1,))
    uni.counters[:3] = torch.tensor([size, size, size])
    L, node_bytes = buf.tree_levels, 256
    for k in (256, 1024, 8192, 32768):
        idxbuf = torch.randint(0, size, (k,), device=dev, generator=gen)
        tdk = torch.rand(k, device=dev, generator=gen)
        hip = timed(lambda: buf._draw(k, None, None))               # enqueue only: two launches, no host read
        uniform = timed(lambda: uni.sample_indices(k))              # the public draw: a host read of len() and torch launches
        hip_public = timed(lambda: buf.sample_prioritized(k))       # the public entries: len(), the draw, five gathers
        uniform_public = timed(lambda: uni.sample_arrays(k))
        tor = timed(lambda: torch_route(pri, size, k, 0.4, gen))
        zero_hits = 0
        if cap == 1 << 24:
            for _ in range(20):
                zero_hits += int((pri[torch_route(pri, size, k, 0.4, gen)[0]] == 0).sum())
            hip_zero = sum(int((pri[buf._draw(k, None, None)[0]] == 0).sum()) for _ in range(20))
        row = {"capacity": cap, "batch": k, "hip_us": hip, "uniform_us": uniform, "torch_route_us": tor, "hip_over_uniform": hip / uniform,
               "hip_public_us": hip_public, "uniform_public_us": uniform_public, "hip_public_over_uniform_public": hip_public / uniform_public,
               "torch_over_hip": tor / hip, "hip_bytes": k * (L * node_bytes + 12) + k * 8,
               "torch_route_bytes": cap * 8 + k * 24}
        if cap == 1 << 24:
            row["torch_route_zero_priority_slots_in_20_draws"], row["hip_zero_priority_slots_in_20_draws"] = zero_hits, hip_zero
        out["sample"].append(row)
        upd = timed(lambda: buf.update_priorities(idxbuf, tdk))
        launches = 1 + sum(1 for l in range(1, L + 1) if -(-cap // 64 ** l) > 64) + 1
        ub = k * (12 + 4) + k * launches * node_bytes
        out["update"].append({"capacity": cap, "batch": k, "us": upd, "launches": launches, "bytes": ub, "floor_us": ub / COPY_FLOOR_TBPS / 1e6,
                              "share_of_copy_floor": ub / COPY_FLOOR_TBPS / 1e6 / upd})
    for count in (4096, 65536):
        if count > cap:
            continue
        before = torch.tensor([cap - count // 2, size, 0, 0], device=dev)      # a push that wraps
        after = torch.tensor([count // 2, size, count, 0], device=dev)
        def push():
            buf._before.copy_(before)
            buf._L.gvec_per_push(0, buf._stream(), buf.tree.data_ptr(), cap, buf._before.data_ptr(), after.data_ptr(), count)
        us = timed(push)
        pb = count * 8 + (count // 64 + 2) * 4 + 32
        out["push"].append({"capacity": cap, "rows": count, "us_with_the_32_byte_copy": us, "launches": 2, "bytes": pb,
                            "floor_us": pb / COPY_FLOOR_TBPS / 1e6, "share_of_copy_floor": pb / COPY_FLOOR_TBPS / 1e6 / us})
    del buf, uni, pri
    torch.cuda.empty_cache()

if not a.no_pool:
    # the resident pool of DESIGN.md 4.6 (15x15, 2 players, a policy that costs nothing), uniform and prioritized alternating
    def policy(states, masks, workers, g):
        return fixed
    out["pool"] = []
    for B in (4096, 65536):
        obs_bytes = 9 * 15 * 15 * 4
        cap = min(max(4 * B, 200000), int(40e9 // (2 * obs_bytes)))
        rates = {"uniform": [], "prioritized": []}
        for rep in range(3):
            for name, cls in (("uniform", DeviceReplayBuffer), ("prioritized", PrioritizedDeviceReplayBuffer)):
                buf = cls(cap)
                pool = ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=15, board_height=15, max_players=2, seed=1, board_pool=1024,
                                                                     device_outputs=True), policy, buf, max_steps_per_episode=200, batched_actions=True)
                fixed = torch.zeros(B, dtype=torch.int64, device=dev)
                pool.collect(1)
                fixed = (pool._mask * torch.rand(pool._mask.shape, device=dev)).argmax(1)
                pool.collect(30)
                torch.cuda.synchronize()
                n = 300
                t0 = time.perf_counter()
                pool.collect(n)
                torch.cuda.synchronize()
                rates[name].append(B * n / (time.perf_counter() - t0))
                pool._env.close()
                del pool, buf
                torch.cuda.empty_cache()
        mu, mp = statistics.median(rates["uniform"]), statistics.median(rates["prioritized"])
        out["pool"].append({"envs": B, "board": "15x15", "ring_capacity": cap, "uniform_transitions_per_s": rates["uniform"],
                            "prioritized_transitions_per_s": rates["prioritized"], "prioritized_over_uniform": mp / mu,
                            "uniform_spread": (max(rates["uniform"]) - min(rates["uniform"])) / mu})
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
