#!/usr/bin/env python3
"""The SpatialDQN collection tick measured on the network and game of notebooks/experiment.ipynb (tools/spatial_bench.py: tagging 1v4,
5 jobs, 9x9, GlobalFeaturizer, n_channels [7, 5, 3], three RNN layers of 64, head [16, 16]) at T = 2 and T = 6:

  (1) the tick of DeviceReplayBuffer.collect with a WindowedPolicyRollout(kernels=True) -- susnet_state_window_push, one susnet_featurize,
      both teams' susnet_spatial_forward, susnet_agent_policy_actions + susnet_step into the feed, and the block's susnet_ring_append --
      against the acting tick WindowedPolicyRollout(kernels=True).step() (featurizer.fit, both forwards, torch argmax / role select /
      epsilon mix / dead mask, env.step, torch.roll / torch.where on the window), each side on its own env of the same seed;
  (2) train() on that policy with a DeviceDQNTeamTrainer(spatial=True) at batch 32: transitions per second, the train steps included.

The two sides of (1) are warmed up, then timed REPEATS times in alternation with a device synchronise at the end of each window of TICKS
ticks; the JSON holds every repeat, the median and the min-max spread.

    python tools/spatial_collect_bench.py [--batch 65536] [--ticks 5] [--repeats 5] [--train-ticks 21] [--out profiles/spatial_collect_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spatial_bench import alternate, notebook_network, sn, summary  # noqa: E402


class Constant:
    def __init__(self, v):
        self.v = v

    def value(self, step):
        return self.v


def game(B, seed=1):
    return sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=B, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                            obs=sn.ObsConfig("raw", dtype=torch.uint8), check_errors=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-ticks", type=int, default=21)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_collect_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spatial_collect_bench needs the MI355X"
    B, eps = args.batch, args.epsilon
    result = {"batch": B, "ticks": args.ticks, "repeats": args.repeats, "epsilon": eps, "device": torch.cuda.get_device_name(0), "rows": []}
    for T in (2, 6):
        envs = [game(B), game(B)]
        A = envs[0].n_agents
        feats = [sn.GlobalFeaturizer(e) for e in envs]
        Fn = envs[0]._make_obs(feats[0].config, 1, rows=1)[2].shape[-1] + A
        imp, crew = notebook_network(envs[0], Fn, envs[0].n_imposter_actions, 3), notebook_network(envs[0], Fn, envs[0].n_crew_actions, 4)
        acting = sn.WindowedPolicyRollout(envs[0], feats[0], imp, crew, sequence_length=T, epsilon=eps, mask_dead=True, kernels=True)
        collecting = sn.WindowedPolicyRollout(envs[1], feats[1], imp, crew, sequence_length=T, mask_dead=True, kernels=True)
        assert acting.spatial_imposter is not None and collecting.spatial_crew is not None
        ring = sn.DeviceReplayBuffer(B * args.ticks, envs[1].flattened_state_size, T, A, envs[1].n_imposters, device=envs[1].device)
        acting.reset()
        envs[1].reset()

        def act_ticks():
            for _ in range(args.ticks):
                acting.step()

        def collect_ticks():
            ring.collect(envs[1], collecting, args.ticks, epsilon=eps, mask_dead=True, ticks_per_append=args.ticks)

        t = alternate({"collect": collect_ticks, "acting_step": act_ticks}, args.repeats)
        row = {"T": T, "rows": B * A, "tick_us": {k: summary([x / args.ticks * 1e6 for x in v]) for k, v in t.items()}}
        row["collect_over_acting"] = row["tick_us"]["collect"]["median"] / row["tick_us"]["acting_step"]["median"]
        if T == 2:  # train() at the reference's default window
            n = args.train_ticks
            trainer = sn.DeviceDQNTeamTrainer(envs[1], imp, crew, [], lr=1e-4, gamma=0.99, policy=collecting, featurizer=feats[1], spatial=True)
            big = sn.DeviceReplayBuffer(B * n, envs[1].flattened_state_size, T, A, envs[1].n_imposters, device=envs[1].device)
            assert trainer.uses_spatial(big)
            gen = torch.Generator(device="cuda:0")
            gen.manual_seed(1)
            with tempfile.TemporaryDirectory() as d:
                for k in range(2):  # (the first run warms up: allocations, the learner's workspace)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sn.train(envs[1], sn.EpisodicMetricHandler(), n, big, collecting, trainer, Constant(eps), os.path.join(d, str(k)),
                             train_step_interval=5, batch_size=32, generator=gen)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
            row["train"] = {"ticks": n, "batch_size": 32, "train_step_interval": 5, "seconds": dt, "transitions_per_s": n * B / dt}
            del trainer, big
        result["rows"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) or k == "train" else {a: round(b["median"], 1) for a, b in v.items()}) for k, v in row.items()}),
              flush=True)
        del envs, feats, acting, collecting, ring
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (after every window length: a run that is cut short keeps what it measured)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
