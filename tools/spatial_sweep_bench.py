"""Microseconds per sweep train step of K SpatialDQN learners (DeviceDQNSweepTrainer -> susnet_spatial_train_sweep: K learners in the
launches of one) against the same K members' own steps one after another (DeviceDQNTeamTrainer -> susnet_spatial_train_step), both teams
trained, on the notebook's network (tools/spatial_train_bench.py: base 1v4, 5 jobs, 9x9, GlobalFeaturizer, T = 6, channels [7, 5, 3] with
the repeated last layer, k = 3, three RNN layers of 64, head [64, 16, 16, n]) at n in {32, 4096} rows and K in {1, 3, 8, 16}.  Both
sides include every member's gather and featurize (the sweep shares none of it).

Method (tools/spatial_train_bench.py's): warm both sides up, then alternate them, 5 windows of --steps steps each, every window timed with
device events around work that ends in a synchronise; reported per side: the median window with (min - max).  `sweep_not_slower` is the
rule the default path rests on: at K = 3, n = 32 the sweep's median is not above the sequential median by more than the spread between
windows the run itself shows (the larger of the two sides' max - min).  Writes the JSON to --out (default
profiles/spatial_sweep_bench.json) and prints it as one line."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from spatial_train_bench import DEV, WINDOWS, alternate, game, models  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
GAMMAS = (0.99, 0.9, 0.8)
GAME = "notebook_global_t6"


def member(k, envs, ticks):
    env, Fz, T, cfg = game(GAME, envs)
    imp, crew = models(env, Fz, cfg)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], 1e-4, GAMMAS[k % 3], featurizer=Fz(env), spatial=True)
    ring = pkg.DeviceReplayBuffer(envs * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, ticks)
    return trainer, ring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="32,4096")
    ap.add_argument("--learners", default="1,3,8,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_sweep_bench.json"))
    args = ap.parse_args()
    Ks = [int(x) for x in args.learners.split(",")]
    members = [member(k, 256, 16) for k in range(max(Ks))]
    agents = members[0][0].env.n_agents
    out = {"unit": "us_per_step_of_K_learners", "device": torch.cuda.get_device_name(0), "game": GAME,
           "method": f"warm-up {args.warmup}, sides alternated, {WINDOWS} windows of {args.steps} steps timed with device events: median (min, max)",
           "launches_per_sweep_step": {str(K): (1 if K <= 8 else 2) + 4 * agents * 2 for K in Ks},
           "launches_per_sequential_step": {str(K): K * (1 + 4 * agents * 2) for K in Ks}, "sizes": {}}
    for n in [int(x) for x in args.sizes.split(",")]:
        idxs = [torch.randint(0, ring.size, (n,), device=DEV) for _, ring in members]
        rows = {}
        for K in Ks:
            trainers, rings = [m[0] for m in members[:K]], [m[1] for m in members[:K]]
            sweep = pkg.DeviceDQNSweepTrainer(trainers)
            assert sweep.uses_spatial(rings)

            def sequential():
                for t, r, i in zip(trainers, rings, idxs):
                    t.train_step_on_indices(r, i)

            r = alternate({"sweep": lambda: sweep.train_step_on_indices(rings, idxs[:K]), "sequential": sequential}, args.steps, args.warmup)
            r["sequential_over_sweep"] = round(r["sequential"]["median"] / r["sweep"]["median"], 2)
            rows[str(K)] = r
            print(n, K, json.dumps(r), flush=True)
        out["sizes"][str(n)] = rows
    r = out["sizes"].get("32", {}).get("3")
    if r is not None:
        spread = max(r["sweep"]["max"] - r["sweep"]["min"], r["sequential"]["max"] - r["sequential"]["min"])
        out["sweep_not_slower_k3_n32"] = {"holds": r["sweep"]["median"] <= r["sequential"]["median"] + spread, "spread_between_windows": round(spread, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
