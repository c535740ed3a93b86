#!/usr/bin/env python3
"""The dense Q-network kernel (susnet_mlp_forward) measured:

  (1) the kernel alone: microseconds per call at n rows, the reference architecture [F, 256, 128, 64, 16, n_actions];
  (2) the policy tick (PolicyRollout.tick: network, argmax / crew draws, step) in env-steps/s on three games no fused path serves --
      base 1v3 9x9 5 jobs, tagging 1v4 9x9 5 jobs, base 2v6 14x14 4 jobs -- with dense=True against dense=False (the torch modules: what
      the tick did before the dense kernel existed: the baseline), and DeviceReplayBuffer.collect with the dense policy on the same games;
  (3) the price of generality: the dense kernel on env.obs against susnet_qnet_forward on the 1v2 14x14 game's compiled-in layout.

Every pair is warmed up, then timed REPEATS times in alternation (a, b, a, b, ...) with a device synchronise at the end of each window;
the JSON holds every repeat, the median and the min-max spread.

    python tools/dense_qnet_bench.py [--batch 65536] [--ticks 200] [--calls 200] [--repeats 5] [--out profiles/dense_qnet_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sn = importlib.import_module("sus-net_amd")

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
COMPS2 = ["onehot_pos", "alive_crew"]


def comps_of(game):
    return COMPS2 if game == "base_2v6_14x14_j4" else COMPS3  # closest_crew is defined with one imposter only (component.py:442-446)


def make_env(game, batch, seed=1):
    kw = dict(batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, obs=sn.ObsConfig("flat", comps_of(game)),
              export_state=False, check_errors=False)
    if game == "base_1v3_9x9_j5":
        return sn.BatchedFourRoomEnv(1, 3, 5, grid_size=9, **kw)
    if game == "tagging_1v4_9x9_j5":
        return sn.BatchedFourRoomEnvWithTagging(1, 4, 5, grid_size=9, **kw)
    if game == "base_2v6_14x14_j4":
        return sn.BatchedFourRoomEnv(2, 6, 4, grid_size=14, **kw)
    if game == "base_1v2_14x14_j4":
        return sn.BatchedFourRoomEnv(1, 2, 4, grid_size=14, **kw)
    raise ValueError(game)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(variants, repeats):
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    return times


def summary(values):
    v = sorted(values)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1], "all": values}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_qnet_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dense_qnet_bench needs the MI355X"
    B = args.batch
    result = {"batch": B, "ticks": args.ticks, "calls": args.calls, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "kernel_alone": [], "policy_tick": [], "collect": [], "against_fused": None}

    for game in ("base_1v3_9x9_j5", "tagging_1v4_9x9_j5", "base_2v6_14x14_j4"):
        env = make_env(game, B)
        env.reset()
        comps = comps_of(game)
        imp = sn.policy.reference_imposter_mlp(env, comps, seed=3)
        crew = sn.policy.reference_crew_mlp(env, comps, seed=4)
        dense = sn.PolicyRollout(env, imp, crew, components=comps, dense=True)
        torch_path = sn.PolicyRollout(env, imp, crew, components=comps, dense=False)
        assert dense.dense_imposter is not None and dense.dense_crew is not None and torch_path.dense_imposter is None
        assert dense.fused_imposter is None, "a game no fused path serves"
        # (1) the kernel alone, and the torch module on the same rows
        net = dense.dense_imposter
        spatial = dense._spatial

        def kernel_calls():
            for _ in range(args.calls):
                net.forward(env.obs)

        def module_calls():
            with torch.no_grad():
                for _ in range(args.calls):
                    imp(spatial, env.obs)

        t = alternate({"dense_kernel": kernel_calls, "torch_module": module_calls}, args.repeats)
        row = {"game": game, "dims": net.dims, "rows": B}
        for k, ts in t.items():
            row[k + "_us_per_call"] = summary([1e6 * x / args.calls for x in ts])
        row["torch_over_dense"] = row["torch_module_us_per_call"]["median"] / row["dense_kernel_us_per_call"]["median"]
        result["kernel_alone"].append(row)
        print(json.dumps(row), flush=True)

        # (2) the policy tick, both teams by their networks
        def ticks_of(pol):
            def run():
                for _ in range(args.ticks):
                    pol.tick()
            return run

        t = alternate({"dense": ticks_of(dense), "torch_modules": ticks_of(torch_path)}, args.repeats)
        row = {"game": game, "batch": B}
        for k, ts in t.items():
            row[k + "_env_steps_per_s"] = summary([args.ticks * B / x for x in ts])
        row["dense_over_torch"] = row["dense_env_steps_per_s"]["median"] / row["torch_modules_env_steps_per_s"]["median"]
        result["policy_tick"].append(row)
        print(json.dumps(row), flush=True)

        # (2b) collect on the same game: per tick susnet_observe + the dense forward(s) + susnet_policy_step, one ring append per block
        # (no torch-module form of collect exists: the figure stands beside the dense tick's, the difference is collect's own overhead)
        ring = sn.DeviceReplayBuffer(B * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)

        def collect_run():
            ring.collect(env, dense, args.ticks, epsilon=0.1, mask_dead=True, ticks_per_append=16)

        t = alternate({"collect": collect_run}, args.repeats)
        row = {"game": game, "batch": B, "ticks_per_append": 16,
               "dense_collect_env_steps_per_s": summary([args.ticks * B / x for x in t["collect"]])}
        result["collect"].append(row)
        print(json.dumps(row), flush=True)
        del env, dense, torch_path, ring

    # (3) against the fused kernel on its own layout
    env = make_env("base_1v2_14x14_j4", B)
    env.reset()
    imp = sn.policy.reference_imposter_mlp(env, COMPS3, seed=3)
    packed = sn.policy.pack_mlp(env, imp, COMPS3)
    net = sn.DenseQNet(env, imp)
    assert packed is not None and net is not None

    def fused_calls():
        for _ in range(args.calls):
            env.qnet_forward(packed)

    def dense_calls():
        for _ in range(args.calls):
            net.forward(env.obs)

    t = alternate({"susnet_qnet_forward": fused_calls, "susnet_mlp_forward": dense_calls}, args.repeats)
    row = {"game": "base_1v2_14x14_j4 (cfg5)", "dims": net.dims, "rows": B}
    for k, ts in t.items():
        row[k + "_us_per_call"] = summary([1e6 * x / args.calls for x in ts])
    row["dense_over_fused"] = row["susnet_mlp_forward_us_per_call"]["median"] / row["susnet_qnet_forward_us_per_call"]["median"]
    result["against_fused"] = row
    print(json.dumps(row), flush=True)

    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
