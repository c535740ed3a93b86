#!/usr/bin/env python3
"""The SpatialDQN forward kernels (susnet_spatial_forward) measured on the network and game of notebooks/experiment.ipynb -- the tagging
game 1v4 with 5 jobs on 9x9, GlobalFeaturizer, n_channels [7, 5, 3], 3x3 / stride 1 / padding 1, three RNN layers of 64, head [16, 16] --
at T = 2 and T = 6:

  (1) one team's forward over all B * A (env, agent) rows: SpatialQNet.forward (two launches) against the torch module in eval mode called
      once per agent view, which is what WindowedPolicyRollout.act() runs without the kernels;
  (2) the whole WindowedPolicyRollout tick (featurize, both teams' networks, argmax, step, window roll) with kernels=True against
      kernels=False.

Every pair is warmed up, then timed REPEATS times in alternation (a, b, a, b, ...) with a device synchronise at the end of each window;
the JSON holds every repeat, the median and the min-max spread.

    python tools/spatial_bench.py [--batch 65536] [--ticks 5] [--calls 3] [--repeats 5] [--out profiles/spatial_bench.json]
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


def notebook_network(env, Fn, n_actions, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = sn.SpatialDQN(input_image_size=env.n_rows, non_spatial_input_size=Fn, n_channels=[env.n_agents + 2, 5, 3], strides=[1, 1], paddings=[1, 1],
                          kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=64, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 16],
                          n_actions=n_actions)
    return m.to(env.device).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spatial_bench needs the MI355X"
    B = args.batch
    result = {"batch": B, "ticks": args.ticks, "calls": args.calls, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "rows": []}
    for T in (2, 6):
        env = sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=B, device="cuda:0", rng="philox", seed=1, auto_reset=True, grid_size=9,
                                               obs=sn.ObsConfig("raw", dtype=torch.uint8), check_errors=False)
        feat = sn.GlobalFeaturizer(env)
        A = env.n_agents
        Fn = env._make_obs(feat.config, 1, rows=1)[2].shape[-1] + A
        imp, crew = notebook_network(env, Fn, env.n_imposter_actions, 3), notebook_network(env, Fn, env.n_crew_actions, 4)
        on = sn.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, kernels=True)
        off = sn.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, kernels=False)
        assert on.spatial_imposter is not None and on.spatial_crew is not None and off.spatial_imposter is None
        on.reset()
        off.window = on.window
        for _ in range(5):
            on.step()
        feat.fit(on.window)
        spatial, non_spatial = on.kernel_inputs()
        views = feat.generate_featurized_states()
        net = on.spatial_imposter

        def kernel_calls():
            for _ in range(args.calls):
                net.forward(spatial, non_spatial, A)

        def module_calls():
            with torch.no_grad():
                for _ in range(args.calls):
                    for sp, ns in views:
                        imp(sp, ns)

        t = alternate({"kernels": kernel_calls, "torch_module": module_calls}, args.repeats)
        row = {"T": T, "rows": B * A, "team_forward_us": {k: summary([x / args.calls * 1e6 for x in v]) for k, v in t.items()}}
        row["kernels_over_torch_forward"] = row["team_forward_us"]["kernels"]["median"] / row["team_forward_us"]["torch_module"]["median"]

        def ticks_of(runner):
            def run():
                runner.window = on.window if runner is off else runner.window
                for _ in range(args.ticks):
                    runner.step()
                if runner is off:
                    on.window = off.window
            return run

        t = alternate({"kernels": ticks_of(on), "torch_module": ticks_of(off)}, args.repeats)
        row["tick_us"] = {k: summary([x / args.ticks * 1e6 for x in v]) for k, v in t.items()}
        row["kernels_over_torch_tick"] = row["tick_us"]["kernels"]["median"] / row["tick_us"]["torch_module"]["median"]
        result["rows"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b["median"], 1) for a, b in v.items()}) for k, v in row.items()}), flush=True)
        del env, feat, on, off, spatial, non_spatial, views
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (after every window length: a run that is cut short keeps what it measured)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
