#!/usr/bin/env python3
"""n-step returns on the device ring (gvec_nstep_*): (a) the one-step baseline `sample_arrays`, (b) the fused
n-step gather for n_step 1 / 3 / 5 - as the public `sample_nstep` and as the gather alone against the five torch gathers over
the same indices, with bytes moved / time against the device-to-device copy rate - over a ring of 15x15 observations filled
by the resident pool, and (c) what linking adds to a collection step.  One process, every shape warmed up, medians of event
timings.  Writes profiles/nstep_bench.json and prints it as one JSON line.

    scripts/bench_nstep.py [--out profiles/nstep_bench.json] [--capacity 1000000] [--reps 20]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_nstep.py --reps 3`."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from generalsreinforcementlearning_amd._lib import CollectArgs, load
from generalsreinforcementlearning_amd.env_pool import ParallelVecEnvPool
from generalsreinforcementlearning_amd.replay import DeviceReplayBuffer
from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_bench.json"))
ap.add_argument("--capacity", type=int, default=1_000_000)
ap.add_argument("--fill-envs", type=int, default=16384)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda", 0)
COPY_FLOOR_TBPS = 6.29                      # the device-to-device copy rate
OBS = (9, 15, 15)
ROW = 9 * 15 * 15 * 4


def timed(fn, reps=a.reps, warm=3, inner=10):
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


out = {"device": torch.cuda.get_device_name(0), "copy_floor_TBps": COPY_FLOOR_TBPS, "board": "15x15", "ring_capacity": a.capacity, "gather": [],
       "link": []}

# ---- the ring: filled (and linked) by the resident pool, a policy that costs nothing ----------------------------------
buf = DeviceReplayBuffer(a.capacity, n_step=5, gamma=0.99)
B = a.fill_envs
fixed = torch.zeros(B, dtype=torch.int64, device=dev)
pool = ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=15, board_height=15, max_players=2, seed=1, board_pool=1024, device_outputs=True),
                          lambda s, m, w, g: fixed, buf, max_steps_per_episode=40, batched_actions=True)
pool.collect(1)
fixed = (pool._mask * torch.rand(pool._mask.shape, device=dev)).argmax(1)
pool.collect(a.capacity // B + 8)
torch.cuda.synchronize()
pool._env.close()
out["ring_fill"], out["ring_linked_share"] = len(buf), float((buf.ring_succ >= 0).double().mean())
out["baseline_note"] = ("sample_arrays_us and torch_gathers_us are timed in this build: DeviceReplayBuffer.sample_arrays is the parent "
                        "commit's code, unchanged, so they stand for (a), the parent's one-step batch")


def view(n):
    """A buffer of n_step n over the SAME ring and links (no copy): what a learner constructing it with n_step=n would hold."""
    v = DeviceReplayBuffer(a.capacity, n_step=n, gamma=0.99)
    for f in ("state", "next_state", "action", "reward", "done", "counters", "obs_shape"):
        setattr(v, f, getattr(buf, f))
    v.ring_succ = buf.ring_succ if n > 1 else None
    return v


for k in (1024, 32768):
    idx = buf.sample_indices(k)
    rows_bytes = k * 4 * ROW                                        # two rows read, two written, per sample
    small = k * (8 + 8 + 8 + 1) * 2                                 # action, reward, done in and out, the index
    a_us = timed(lambda: buf.sample_arrays(k))                      # (a): len(), the draw, five torch gathers
    torch_us = timed(lambda: (buf.state[idx], buf.action[idx], buf.reward[idx], buf.next_state[idx], buf.done[idx]))
    for n in (1, 3, 5):
        v = view(n)
        pub = timed(lambda: v.sample_nstep(k))                      # (b): len(), the draw, ONE launch
        hip = timed(lambda: v._gather_nstep(idx))
        steps = v._gather_nstep(idx)["steps"].double().mean().item()
        nbytes = rows_bytes + small + k * (8 + 4 + 8 + 8) + int(k * (steps - 1) * (8 + 8 + 1))
        out["gather"].append({"batch": k, "n_step": n, "mean_steps": steps, "sample_arrays_us": a_us, "sample_nstep_us": pub,
                              "sample_nstep_over_sample_arrays": pub / a_us, "torch_gathers_us": torch_us, "gather_us": hip,
                              "gather_over_torch_gathers": hip / torch_us, "bytes": nbytes, "TBps": nbytes / hip / 1e6,
                              "share_of_copy_floor": nbytes / hip / 1e6 / COPY_FLOOR_TBPS})
del buf, pool, v
torch.cuda.empty_cache()

# ---- (c) a collection step with and without the links: the handle-free calls on fixed per-step tensors, every worker live ----
L = load()
F = 9 * 15 * 15
for B in (4096, 65536):
    cap = 4 * B
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    t = dict(state=torch.rand(B, F, device=dev), next_state=torch.rand(B, F, device=dev), action=z(B, torch.int64), reward=torch.rand(B, device=dev).double(),
             terminated=(torch.rand(B, device=dev) < 0.02).to(torch.uint8), truncated=z(B, torch.uint8), was_reset=z(B, torch.uint8), needs_reset=z(B, torch.uint8),
             ring_state=z((cap, F), torch.float32), ring_next_state=z((cap, F), torch.float32), ring_action=z(cap, torch.int64),
             ring_reward=z(cap, torch.float64), ring_done=z(cap, torch.uint8), ring_counters=z(4, torch.int64), episode_reward=z(B, torch.float64),
             episode_length=z(B, torch.int64), pool_counters=z(4, torch.int64),
             scratch=z((int(L.gvec_pool_collect_scratch_bytes(B)) + 7) // 8, torch.int64))
    args = CollectArgs()
    args.num_envs, args.obs_floats, args.max_steps_per_episode, args.capacity, args.result_capacity = B, F, 200, cap, 0
    for name, tensor in t.items():
        setattr(args, name, tensor.data_ptr())
    before, succ, last = z(4, torch.int64), torch.full((cap,), -1, dtype=torch.int64, device=dev), torch.full((B, 2), -1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def collect():
        assert L.gvec_pool_collect(0, stream, ctypes.byref(args)) == 0

    def collect_and_link():
        before.copy_(t["ring_counters"])
        assert L.gvec_pool_collect(0, stream, ctypes.byref(args)) == 0
        assert L.gvec_nstep_link(0, stream, ctypes.byref(args), before.data_ptr(), succ.data_ptr(), last.data_ptr()) == 0

    rounds = [(timed(collect), timed(collect_and_link)) for _ in range(3)]     # alternating: drift shows as spread
    c, cl = statistics.median(r[0] for r in rounds), statistics.median(r[1] for r in rounds)
    out["link"].append({"envs": B, "collect_us": c, "collect_and_link_us": cl, "added_us": cl - c, "added_share": (cl - c) / c,
                        "collect_rounds_us": [r[0] for r in rounds], "collect_and_link_rounds_us": [r[1] for r in rounds],
                        "link_bytes": B * (1 + 16 + 16 + 8 + 8)})
    del t, succ, last
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
