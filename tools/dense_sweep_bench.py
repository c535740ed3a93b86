"""Microseconds per sweep train step of K dense learners (DeviceDQNSweepTrainer -> susnet_mlp_train_sweep: K learners in the launches of
one) against the same K members' own steps one after another (DeviceDQNTeamTrainer(dense=True) -> susnet_mlp_train_step), both teams
trained, at n in {32, 4096} rows and K in {1, 3, 8, 16}, on three cases:
  notebook_t1  base 1v3, 5 jobs, 9x9, onehot_pos + alive_crew + closest_crew, the notebook's stack [F, 256, 128, 64, 16, n_actions], T = 1
  notebook_t2  the same at the reference's default window, T = 2: [2 F, 256, 128, 64, 16, n_actions]
  cfg5_short   bench.py's cfg5 layout (1v2, 4 jobs, 14x14, the same components: F = 88) with a stack the fused learner does not serve,
               [F, 128, 64, n_actions]
Both sides include every member's gather and featurize (the sweep shares none of it).

Method (tools/spatial_sweep_bench.py's): warm both sides up, then alternate them, 5 windows of --steps steps each, every window timed with
device events around work that ends in a synchronise; reported per side: the median window with (min - max).  No ratio is asserted:
`sweep_not_faster` lists every (case, n, K) whose sweep median is not below the sequential median.  --cases runs a subset and merges it
into an --out that already holds other cases of the same method (so each case can run as a process of its own, under its own time limit).
Writes the JSON to --out (default profiles/dense_sweep_bench.json) and prints it as one line."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from spatial_train_bench import DEV, WINDOWS, alternate  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
GAMMAS = (0.99, 0.9, 0.8)
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
CASES = {"notebook_t1": ("base9_1v3", 1, [256, 128, 64, 16]), "notebook_t2": ("base9_1v3", 2, [256, 128, 64, 16]), "cfg5_short": ("base14_1v2", 1, [128, 64])}


def member(case, k, envs, ticks):
    game, T, hidden = CASES[case]
    kw = dict(batch=envs, device=DEV, rng="philox", auto_reset=True, check_errors=False, shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3))
    env = pkg.BatchedFourRoomEnv(1, 3, 5, seed=3 + k, grid_size=9, **kw) if game == "base9_1v3" else pkg.BatchedFourRoomEnv(1, 2, 4, seed=5 + k, grid_size=14, **kw)
    F = env.obs.shape[-1]
    torch.manual_seed(10 + k)
    imp, crew = pkg.MLP([T * F, *hidden, env.n_imposter_actions]), pkg.MLP([T * F, *hidden, env.n_crew_actions])
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew, COMPS3, 1e-4, GAMMAS[k % 3], dense=True, sequence_length=T)
    ring = pkg.DeviceReplayBuffer(envs * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, ticks)
    return trainer, ring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="32,4096")
    ap.add_argument("--learners", default="1,3,8,16")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_sweep_bench.json"))
    args = ap.parse_args()
    Ks = [int(x) for x in args.learners.split(",")]
    out = {"unit": "us_per_step_of_K_learners", "device": torch.cuda.get_device_name(0),
           "method": f"warm-up {args.warmup}, sides alternated, {WINDOWS} windows of {args.steps} steps timed with device events: median (min, max)",
           "cases": {}}
    if os.path.exists(args.out):
        old = json.load(open(args.out))
        if old.get("method") == out["method"] and old.get("device") == out["device"]:
            out["cases"] = old.get("cases", {})
    for case in args.cases.split(","):
        members = [member(case, k, 256, 16) for k in range(max(Ks))]
        first = members[0][0]
        agents = first.env.n_agents
        got = {"game": CASES[case][0], "T": CASES[case][1], "dims": first._dense_dims, "agents": agents,
               "launches_per_sweep_step": 1 + 2 * agents * 2, "launches_per_sequential_step": {str(K): K * (1 + 2 * agents * 2) for K in Ks}, "sizes": {}}
        for n in [int(x) for x in args.sizes.split(",")]:
            idxs = [torch.randint(0, ring.size, (n,), device=DEV) for _, ring in members]
            rows = {}
            for K in Ks:
                trainers, rings = [m[0] for m in members[:K]], [m[1] for m in members[:K]]
                sweep = pkg.DeviceDQNSweepTrainer(trainers)
                assert sweep.uses_dense(rings) and not sweep.uses_hip(rings)

                def sequential():
                    for t, r, i in zip(trainers, rings, idxs):
                        t.train_step_on_indices(r, i)

                r = alternate({"sweep": lambda: sweep.train_step_on_indices(rings, idxs[:K]), "sequential": sequential}, args.steps, args.warmup)
                r["sequential_over_sweep"] = round(r["sequential"]["median"] / r["sweep"]["median"], 2)
                rows[str(K)] = r
                print(case, n, K, json.dumps(r), flush=True)
            got["sizes"][str(n)] = rows
        out["cases"][case] = got
        del members
    out["sweep_not_faster"] = [f"{case} n={n} K={K}" for case, c in out["cases"].items() for n, rows in c["sizes"].items() for K, r in rows.items()
                               if r["sweep"]["median"] >= r["sequential"]["median"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
