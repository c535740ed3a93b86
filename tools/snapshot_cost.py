#!/usr/bin/env python3
"""What one snapshot of a training run costs (``run_experiment(snapshot_interval=...)``: ``run_state.pt``), at two configurations:

  cfg5     bench.py's cfg5 game (1v2, 14x14, 4 jobs, the reference MLPs, both teams trained), 65 536 envs, a ring of 100 000 rows
  spatial  the notebook's game and network (tagging 1v4, 5 jobs, 9x9, GlobalFeaturizer, three RNN layers of 64), T = 2, 65 536 envs, a ring
           of 100 000 rows

Each run is taken to its second block boundary with ``stop_after=6`` (the ring is full by then), then two things are timed on the stopped
run, warmed up and REPEATS times in alternation with a device synchronise around each: (a) ``state_dict()`` alone -- the wait for the
device and the copies to the host -- and (b) ``snapshot()`` -- the same plus ``torch.save`` to a temporary name, fsync and ``os.replace``.
The JSON holds every repeat, the medians, the min-max spread and the file's size.  The episode log grows by 56 bytes per finished episode
(at most 2^20 of them): the sizes here are those of a young run.

    python tools/snapshot_cost.py [--batch 65536] [--ring 100000] [--repeats 5] [--out profiles/snapshot_cost.json]
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spatial_bench import alternate, notebook_network, sn, summary  # noqa: E402

COMPS = ["onehot_pos", "alive_crew", "closest_crew"]


def cfg5(B):
    env = sn.BatchedFourRoomEnv(1, 2, 4, batch=B, device="cuda:0", rng="philox", seed=1, auto_reset=True, grid_size=14,
                                obs=sn.ObsConfig("flat", COMPS), export_state=False, check_errors=False)
    return env, sn.policy.reference_imposter_mlp(env, COMPS, seed=3), sn.policy.reference_crew_mlp(env, COMPS, seed=4), dict(components=COMPS)


def spatial(B):
    env = sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=B, device="cuda:0", rng="philox", seed=1, auto_reset=True, grid_size=9,
                                           obs=sn.ObsConfig("raw", dtype=torch.uint8), check_errors=False)
    fz = sn.GlobalFeaturizer(env)
    Fn = env._make_obs(fz.config, 1, rows=1)[2].shape[-1] + env.n_agents
    return (env, notebook_network(env, Fn, env.n_imposter_actions, 3), notebook_network(env, Fn, env.n_crew_actions, 4),
            dict(components=[], sequence_length=2, featurizer=fz))


def stopped_run(build, B, ring_rows, base):
    """``run_experiment`` on ``build``'s env and models, stopped at 6 completed ticks: the ``_Run`` it drove."""
    tl, seen = sn.train_loop, []
    real = tl._Run

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append(self)

    env, imp, crew, kw = build(B)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    tl._Run = Spy
    try:
        sn.run_experiment(env, 11, imp, crew, replay_buffer_size=ring_rows, replay_prepopulate_steps=2, batch_size=32, experiment_base_dir=base,
                          generator=gen, stop_after=6, **kw)
    finally:
        tl._Run = real
    return seen[0]


def tensor_bytes(x):
    if torch.is_tensor(x):
        return x.numel() * x.element_size()
    if isinstance(x, dict):
        return sum(tensor_bytes(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return sum(tensor_bytes(v) for v in x)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ring", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "snapshot_cost needs the MI355X"
    result = {"batch": args.batch, "ring_rows": args.ring, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "rows": []}
    for name, build in (("cfg5", cfg5), ("spatial", spatial)):
        with tempfile.TemporaryDirectory() as d:
            run = stopped_run(build, args.batch, args.ring, pathlib.Path(d))
            path = run.save_dir / sn.train_loop.RUN_STATE_FILE
            t = alternate({"state_dict": lambda: run.state_dict(6, 2), "snapshot": lambda: run.snapshot(6, 2)}, args.repeats)
            state = run.state_dict(6, 2)
            row = {"config": name, "file_bytes": path.stat().st_size, "ms": {k: summary([x * 1e3 for x in v]) for k, v in t.items()},
                   "tensor_bytes": {k: tensor_bytes(state[k]) for k in ("env", "ring", "trainer", "policy", "episode_log", "losses")},
                   "episodes_logged": int(state["episode_log"]["counters"][0]), "ring_size": run.ring.size}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            del run, state
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
