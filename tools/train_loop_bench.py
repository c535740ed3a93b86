#!/usr/bin/env python3
"""The device training loop on BASELINE config 5's game (1v2, 14x14, 4 jobs, the reference MLP for both teams): transitions/s of

  (a) collect + train_step alone        -- the loop without any episode bookkeeping (what the primitives give): the baseline
  (b) susnet_amd.train()                -- the same loop with the episode bookkeeping by susnet_episode_stats (EpisodeLog)
  (c) the loop of (a) with the bookkeeping done by torch ops on the feed block, tick by tick, with a host-visible nonzero per block

at train_step_interval = 5, for each batch size given.  Every variant is warmed up, then timed REPEATS times in alternation (a, b, c, a, b,
c, ...) with a device synchronise at the end of each window; the JSON holds every repeat, the median and the min-max spread.

    python tools/train_loop_bench.py [--batch 65536] [--steps 5001] [--repeats 5] [--batch-sizes 32,65536] [--out profiles/train_loop_bench.json]
    python tools/train_loop_bench.py --updates-only 200     # only EpisodeLog.update calls on a collected block: for rocprofv3 --kernel-trace --stats
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import susnet_amd as sn  # noqa: E402

COMPS = ["onehot_pos", "alive_crew", "closest_crew"]
K = 5  # train_step_interval


def setup(batch, seed=1):
    env = sn.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=14,
                                obs=sn.ObsConfig("flat", COMPS), export_state=False, check_errors=False)
    imp = sn.policy.reference_imposter_mlp(env, COMPS, seed=3)
    crew = sn.policy.reference_crew_mlp(env, COMPS, seed=4)
    policy = sn.PolicyRollout(env, imp, crew, components=COMPS, mask_dead=True)
    trainer = sn.DeviceDQNTeamTrainer(env, imp, crew, COMPS, lr=1e-4, gamma=0.99, policy=policy)
    ring = sn.DeviceReplayBuffer(batch * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 8)
    return env, policy, trainer, ring


def primitives_loop(env, policy, trainer, ring, sched, num_steps, batch_size, save_dir, bookkeeping=None):
    """train()'s block loop by hand, with its final checkpoint; ``bookkeeping(feed, n)`` after each collect."""
    env.reset()
    for blk in sn.plan_blocks(num_steps, K, 10_000, 1):
        if blk.sync_ticks:
            trainer.sync_targets()
        ring.collect(env, policy, blk.n_ticks, epsilon=float(sched.value(blk.t0)), ticks_per_append=blk.n_ticks)
        if bookkeeping is not None:
            bookkeeping(*ring.last_feed)
        if blk.trains:
            trainer.train_step(ring, batch_size)
    sn.train_loop._save(trainer.models, save_dir, "100%")


class TorchBookkeeping:
    """The bookkeeping of train.py:385-450 in torch ops on the feed block: per tick G = r + gamma G, the teams' means where an episode
    ended, and the records of the block appended on the host (a nonzero per block: one synchronisation)."""

    def __init__(self, env, gamma):
        B, A = env.batch, env.n_agents
        self.G = torch.zeros(B, A, dtype=torch.float64, device=env.device)
        self.t_episode = torch.zeros(B, dtype=torch.int32, device=env.device)
        self.gamma, self.bits = gamma, (1 << torch.arange(A, device=env.device)).to(torch.int32)
        self.returns, self.lengths = [], []

    def __call__(self, feed, n):
        out = []
        for t in range(n):
            self.G = feed["rewards"][t].to(torch.float64) + self.gamma * self.G
            ended = feed["done"][t] | feed["truncated"][t]
            imp = (feed["roles"][t].to(torch.int32).unsqueeze(1) & self.bits) != 0
            n_imp = imp.sum(1)
            ret_i = (self.G * imp).sum(1) / n_imp
            ret_c = (self.G * ~imp).sum(1) / (imp.shape[1] - n_imp)
            out.append(torch.stack([ret_i, ret_c, (self.t_episode + 1).to(torch.float64), ended.to(torch.float64)], 1))
            self.G = torch.where(ended.unsqueeze(1), torch.zeros_like(self.G), self.G)
            self.t_episode = torch.where(ended, torch.zeros_like(self.t_episode), self.t_episode + 1)
        block = torch.cat(out)
        rows = block[block[:, 3].nonzero().squeeze(1)]  # host-visible size: the synchronisation
        self.returns.append(rows[:, :2])
        self.lengths.append(rows[:, 2])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5001)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-sizes", default="32,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loop_bench.json"))
    ap.add_argument("--updates-only", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_loop_bench needs the MI355X"
    env, policy, trainer, ring = setup(args.batch)
    sched = sn.ExponentialSchedule(1.0, 0.05, 1_000_000)

    if args.updates_only:
        ring.collect(env, policy, K, epsilon=0.5, ticks_per_append=K)
        feed, n = ring.last_feed
        log = sn.EpisodeLog(env, gamma=0.99)
        for _ in range(args.updates_only):
            log.update(feed, n)
        torch.cuda.synchronize()
        print(json.dumps({"updates": args.updates_only, "block_ticks": n, "batch": args.batch, "episodes_logged": log.records()["count"]}))
        return

    result = {"game": "1v2 14x14 4 jobs, MLP [88,256,128,64,16,7] / [..,6], both teams trained", "batch": args.batch, "train_step_interval": K,
              "num_steps": args.steps, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "rows": []}
    tmp_dir = tempfile.TemporaryDirectory()
    tmp = pathlib.Path(tmp_dir.name)
    for bs in (int(v) for v in args.batch_sizes.split(",")):
        def run_a():
            primitives_loop(env, policy, trainer, ring, sched, args.steps, bs, tmp)

        def run_b():
            sn.train(env, sn.EpisodicMetricHandler(), args.steps, ring, policy, trainer, sched, tmp, train_step_interval=K, batch_size=bs,
                     num_saves=1, target_update_interval=10_000)

        def run_c():
            primitives_loop(env, policy, trainer, ring, sched, args.steps, bs, tmp, bookkeeping=TorchBookkeeping(env, 0.99))

        variants = {"a_collect_train_step": run_a, "b_train_with_episode_kernel": run_b, "c_torch_bookkeeping": run_c}
        for fn in variants.values():  # warm-up: every shape, workspace and code object of the timed windows
            fn()
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        trans = args.steps * args.batch
        row = {"batch_size": bs}
        for k, ts in times.items():
            rates = sorted(trans / t for t in ts)
            row[k] = {"transitions_per_s_median": statistics.median(rates), "min": rates[0], "max": rates[-1], "seconds": ts}
        row["b_over_a"] = row["b_train_with_episode_kernel"]["transitions_per_s_median"] / row["a_collect_train_step"]["transitions_per_s_median"]
        row["b_over_c"] = row["b_train_with_episode_kernel"]["transitions_per_s_median"] / row["c_torch_bookkeeping"]["transitions_per_s_median"]
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    A = env.n_agents
    result["episode_kernel_bytes_per_block"] = K * args.batch * (4 * A + 4)  # rewards + done + truncated + roles
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    tmp_dir.cleanup()


if __name__ == "__main__":
    main()
