#!/usr/bin/env python3
"""Host cost of one env.step of the two gym vector envs in device mode: 20x20 boards, 4 players, at 256 envs (the launch and
the Python around it dominate) and at 4,096.  A fixed action tensor, 200 warm-up steps, then 2,000 env.step calls and one
synchronize; microseconds per step.  With `--what pool`: one vector step of a resident ParallelVecEnvPool (the policy call, env.step
and the ring's append) at 256 envs, into a uniform n_step=1 ring and into a prioritized n_step=3 ring, measured the same way.

  scripts/bench_gym_env_host.py [--tree DIR]        one run: a JSON line {"vec/256": us, "vec/4096": us, "selfplay/256": ...}
                                                    with the package imported from DIR (default: this checkout)
  scripts/bench_gym_env_host.py --ab PARENT_TREE [--what pool] [--out FILE] [--runs 5]
        two Python layers over ONE built library (GVEC_LIB, default this checkout's): a checkout of the parent commit and this
        one, a fresh process per run, alternating, each under its own time limit.  Writes every run, the medians and the
        verdict: per env and batch size, median(branch) <= median(parent) + 2 * (max - min of the parent's runs).
        Exit status 1 when a case is above its margin.
"""
import argparse, json, os, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, SIZES = 200, 2000, (256, 4096)


def one_run(tree):
    sys.path.insert(0, tree)
    import torch
    from generalsreinforcementlearning_amd.selfplay_env import GeneralsSelfPlayVecEnv
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    res = {}
    for name, cls in (("vec", GeneralsVecEnv), ("selfplay", GeneralsSelfPlayVecEnv)):
        for B in SIZES:
            env = cls(B, board_width=20, board_height=20, max_players=4, device_outputs=True)
            _, info = env.reset(seed=3)
            acts = torch.argmax(info["valid_actions_mask"].to(torch.uint8), dim=-1)      # the first valid action, kept for every step
            for _ in range(WARMUP):
                env.step(acts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                env.step(acts)
            torch.cuda.synchronize()
            res[f"{name}/{B}"] = round((time.perf_counter() - t0) / STEPS * 1e6, 3)
            env.close()
    print(json.dumps(res), flush=True)


def one_pool_run(tree):
    sys.path.insert(0, tree)
    import torch
    from generalsreinforcementlearning_amd.env_pool import DeviceReplayBuffer, ParallelVecEnvPool, PrioritizedDeviceReplayBuffer
    from generalsreinforcementlearning_amd.vector_env import GeneralsVecEnv
    B, res = SIZES[0], {}
    for name, cls, kw in (("pool/uniform_n1", DeviceReplayBuffer, {}), ("pool/prioritized_n3", PrioritizedDeviceReplayBuffer, {"n_step": 3})):
        fixed = torch.zeros(B, dtype=torch.int64, device="cuda")
        pool = ParallelVecEnvPool(B, lambda n: GeneralsVecEnv(n, board_width=20, board_height=20, max_players=4, seed=3, device_outputs=True),
                                  lambda states, masks, workers, generator: fixed, cls(64 * B, **kw), batched_actions=True)
        pool.collect(1)
        fixed = torch.argmax(pool._mask.to(torch.uint8), dim=-1)                          # the first valid action, kept for every step
        pool.collect(WARMUP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.collect(STEPS)
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t0) / STEPS * 1e6, 3)
        pool._env.close()
    print(json.dumps(res), flush=True)


def ab(parent, out, runs, limit, what):
    env = dict(os.environ, GVEC_LIB=os.environ.get("GVEC_LIB") or os.path.join(HERE, "generalsreinforcementlearning_amd", "libgvec_hip.so"))
    trees = {"parent": os.path.abspath(parent), "branch": HERE}
    rec = {"what": __doc__.split("\n\n")[0], "library": "one build for both (GVEC_LIB)", "unit": "us per pool step" if what == "pool" else "us per env.step",
           "warmup": WARMUP, "steps": STEPS, "runs": {"parent": [], "branch": []}}
    for _ in range(runs):
        for side, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--what", what], env=env, timeout=limit, check=True,
                               stdout=subprocess.PIPE, text=True)
            rec["runs"][side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, rec["runs"][side][-1], flush=True)
    rec["cases"], ok = {}, True
    for case in rec["runs"]["parent"][0]:
        pa, br = ([r[case] for r in rec["runs"][s]] for s in ("parent", "branch"))
        c = {"parent_median": statistics.median(pa), "branch_median": statistics.median(br), "parent_spread": round(max(pa) - min(pa), 3)}
        c["limit"] = round(c["parent_median"] + 2 * c["parent_spread"], 3)
        c["within"] = c["branch_median"] <= c["limit"]
        ok &= c["within"]
        rec["cases"][case] = c
        print(case, c, flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--ab", metavar="PARENT_TREE")
    ap.add_argument("--what", choices=("env", "pool"), default="env")
    ap.add_argument("--out", help="default: profiles/gym_env_host_overhead.json, or profiles/pool_host_overhead.json with --what pool")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per process")
    a = ap.parse_args()
    out = a.out or os.path.join(HERE, "profiles", ("pool" if a.what == "pool" else "gym_env") + "_host_overhead.json")
    sys.exit(ab(a.ab, out, a.runs, a.limit, a.what) if a.ab else (one_pool_run if a.what == "pool" else one_run)(a.tree))
