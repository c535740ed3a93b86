"""Microseconds per train step of ONE trainer object on its two paths: the dense HIP step (susnet_mlp_train_step,
DeviceDQNTeamTrainer(dense=True)) against the torch path (torch_train_step) on games no compiled-in layout serves -- base 1v3 9x9 with 5 jobs
(onehot_pos + alive_crew + closest_crew, both teams), tagging 1v4 9x9 with 5 jobs (onehot_pos, imposters only), ITG 1v10 (onehot_pos, both
teams: 22 updates per step) -- and, on the 1v2 14x14 layout of the fused learner, against susnet_dqn_train_step.  All networks are the
reference stack [F, 256, 128, 64, 16, n_actions].

Method: warm both sides up, then alternate them, 5 windows of --steps steps each; reported per side: the median window
with (min - max).  Writes the JSON to --out (default profiles/dense_train_bench.json) and prints it as one line."""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
DEV = "cuda:0"
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
WINDOWS = 5


def game(name, batch):
    """-> (env, components, crew trained)"""
    kw = dict(batch=batch, device=DEV, rng="philox", auto_reset=True, check_errors=False)
    if name == "base_1v3_j5":
        return pkg.BatchedFourRoomEnv(1, 3, 5, seed=3, grid_size=9, shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3), **kw), COMPS3, True
    if name == "tagging_1v4_j5":
        return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, seed=4, grid_size=9, obs=pkg.ObsConfig("flat", ["onehot_pos"]), **kw), ["onehot_pos"], False
    if name == "itg_1v10":
        itg = dict(n_crew=10, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
        return pkg.BatchedImposterTrainingGround(**itg, grid=pkg.four_room_grid(9, False), seed=6, obs=pkg.ObsConfig("flat", ["onehot_pos"]), **kw), \
            ["onehot_pos"], True
    assert name == "base14_1v2_j4"
    return pkg.BatchedFourRoomEnv(1, 2, 4, seed=5, grid_size=14, shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3), **kw), COMPS3, True


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def alternate(sides, steps, warmup):
    """sides: {name: fn} -> {name: {median, min, max}} over WINDOWS alternating windows."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in sides}
    for _ in range(WINDOWS):
        for k, fn in sides.items():
            got[k].append(window(fn, steps))
    return {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8,32,4096,65536")
    ap.add_argument("--games", default="base_1v3_j5,tagging_1v4_j5,itg_1v10,base14_1v2_j4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_train_bench.json"))
    args = ap.parse_args()
    out = {"unit": "us_per_train_step", "method": f"warm-up {args.warmup}, sides alternated, {WINDOWS} windows of {args.steps} steps: median (min, max)",
           "device": torch.cuda.get_device_name(0), "games": {}}
    for name in args.games.split(","):
        env, comps, crew = game(name, 4096)
        ring = pkg.DeviceReplayBuffer(4096 * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
        ring.populate_fused(env, 16)
        imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
        cr = pkg.policy.reference_crew_mlp(env, comps, seed=4) if crew else None
        dense = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-4, 0.9, train_crew=crew, dense=True)
        other = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, 1e-4, 0.9, train_crew=crew)
        fused = other.uses_hip(ring)  # the compiled-in layout: the dense step (fused step switched off) against susnet_dqn_train_step
        if fused:
            dense.hip = False
        assert dense.uses_dense(ring) and not other.uses_dense(ring)
        against = "susnet_dqn_train_step" if fused else "torch"
        rows = {}
        for n in [int(x) for x in args.sizes.split(",")]:
            idx = torch.randint(0, ring.size, (n,), device=DEV)
            r = alternate({"dense": lambda: dense.train_step_on_indices(ring, idx), against: lambda: other.train_step_on_indices(ring, idx)},
                          args.steps, args.warmup)
            r["dense_speedup"] = round(r[against]["median"] / r["dense"]["median"], 2)
            rows[str(n)] = r
            print(name, n, json.dumps(r), flush=True)
        out["games"][name] = {"agents": env.n_agents, "components": comps, "teams_trained": 2 if crew else 1, "dims": dense._dense_dims[0],
                              "against": against, "sizes": rows}
        del env, ring, dense, other
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
