"""Microseconds per sweep train step (DeviceDQNSweepTrainer -> susnet_dqn_train_sweep, K learners in the launches of one) against K
sequential single-learner steps (DeviceDQNTeamTrainer -> susnet_dqn_train_step) on the same members, for the 1v1 onehot_pos game
(imposter only: the notebooks' sweeps) and 1v2 with both teams, N in {8, 32, 4096}, K in {1, 2, 4, 8, 16}; plus the block cadence: K
5-tick collects and one step at batch 32.  Each variant is warmed up, then the two are timed in alternation `--rounds` times (a round =
`--steps` calls ending in a device synchronise); reported are the median and the range over the rounds, and the two acceptance
conditions: at K = 8, N in {8, 32} the sweep's slowest round is below the sequential loop's fastest; at K = 1 the two ranges overlap.
Prints one JSON line (and writes it to --out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
GAMMAS = (0.99, 0.9, 0.8)


def member(name, batch, seed, ring_ticks, gamma):
    if name == "1v2":
        env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=14,
                                     shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3), check_errors=False)
        comps, crew = COMPS3, True
    else:
        kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
        env = pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device="cuda:0", rng="philox", seed=seed,
                                                auto_reset=True, obs=pkg.ObsConfig("flat", ["onehot_pos"]), check_errors=False)
        comps, crew = ["onehot_pos"], False
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=seed)
    cr = pkg.policy.reference_crew_mlp(env, comps, seed=seed + 100) if crew else None
    policy = pkg.PolicyRollout(env, imp, cr, comps)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-4, gamma, train_crew=crew, policy=policy)
    ring = pkg.DeviceReplayBuffer(batch * ring_ticks, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    return env, policy, trainer, ring


def alternate(variants, steps, warmup, rounds):
    """{name: {"median", "min", "max"}} in us per call: every variant warmed up, then `rounds` rounds with the variants in alternation."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    return {name: {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="8,32,4096")
    ap.add_argument("--learners", default="1,2,4,8,16")
    ap.add_argument("--cadence-learners", default="1,4,8")
    ap.add_argument("--cadence-envs", type=int, default=65536)
    ap.add_argument("--out")
    args = ap.parse_args()
    Ks = [int(x) for x in args.learners.split(",")]
    out = {"unit": "us_per_call", "device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds, "games": {}, "acceptance": {}}
    for name in ("1v1", "1v2"):
        members = [member(name, 1024, 11 + k, 16, GAMMAS[k % 3]) for k in range(max(Ks))]
        for env, _, _, ring in members:
            ring.populate_fused(env, 16)
        rows = {}
        for n in [int(x) for x in args.sizes.split(",")]:
            idxs = [torch.randint(0, m[3].size, (n,), device="cuda:0") for m in members]
            rows[str(n)] = {}
            for K in Ks:
                trainers, rings = [m[2] for m in members[:K]], [m[3] for m in members[:K]]
                sweep = pkg.DeviceDQNSweepTrainer(trainers)
                assert sweep.uses_hip(rings)

                def sequential():
                    for t, r, i in zip(trainers, rings, idxs):
                        t.train_step_on_indices(r, i)
                r = alternate({"sweep": lambda: sweep.train_step_on_indices(rings, idxs[:K]), "sequential": sequential}, args.steps, args.warmup,
                              args.rounds)
                r["sequential_over_sweep"] = round(r["sequential"]["median"] / r["sweep"]["median"], 2)
                rows[str(n)][str(K)] = r
                if K == 8 and n in (8, 32):
                    out["acceptance"][f"{name}_n{n}_k8_sweep_max_below_sequential_min"] = r["sweep"]["max"] < r["sequential"]["min"]
                if K == 1:
                    out["acceptance"][f"{name}_n{n}_k1_ranges_overlap"] = (r["sweep"]["min"] <= r["sequential"]["max"]
                                                                          and r["sequential"]["min"] <= r["sweep"]["max"])
        out["games"][name] = rows
        del members
    # the block cadence on 1v2: K 5-tick collects (one after another on the one stream) + one train step at batch 32
    cad = {}
    cadK = [int(x) for x in args.cadence_learners.split(",")]
    members = [member("1v2", args.cadence_envs, 31 + k, 10, GAMMAS[k % 3]) for k in range(max(cadK))]
    for env, policy, _, ring in members:
        env.reset()
        ring.collect(env, policy, 5, ticks_per_append=5)
    for K in cadK:
        ms = members[:K]
        sweep = pkg.DeviceDQNSweepTrainer([m[2] for m in ms])
        rings = [m[3] for m in ms]

        def collects():
            for env, policy, _, ring in ms:
                ring.collect(env, policy, 5, ticks_per_append=5)

        def block_sweep():
            collects()
            sweep.train_step(rings, 32)

        def block_sequential():
            collects()
            for _, _, trainer, ring in ms:
                trainer.train_step(ring, 32)
        r = alternate({"sweep": block_sweep, "sequential": block_sequential, "collects_only": collects}, max(5, args.steps // 2), 2, args.rounds)
        r["sequential_over_sweep"] = round(r["sequential"]["median"] / r["sweep"]["median"], 2)
        cad[str(K)] = r
    out[f"cadence_1v2_{args.cadence_envs}_envs_5_ticks_plus_step_b32"] = cad
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
