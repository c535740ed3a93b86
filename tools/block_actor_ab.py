"""The acting loop of collect / evaluate / train() under two versions of the Python package, side by side in ONE process on one built
library: the way profiles/block_actor_ab.json was measured when the loop became policy.BlockActor (no kernel changed, so the comparison
is of host code).  ``--parent DIR`` holds the other version's package, e.g.

    mkdir /tmp/parent && git archive <commit> sus-net_amd | tar -x -C /tmp/parent
    python tools/block_actor_ab.py --parent /tmp/parent [--builds 2] [--only b64] [--out profiles/block_actor_ab_run.json]

(a DIR without a built library uses this tree's).  Workloads: the collect shapes of tools/train_loop_bench.py (variant b),
tools/dense_qnet_bench.py, tools/window_bench.py, tools/spatial_collect_bench.py and bench.py's collect_into_replay_ring at 65 536 envs
(bound by the device), and the same loops and evaluate() at 64 envs (bound by the host: where a per-tick Python cost shows).  Every
workload is built ``--builds`` times per package on its own envs, networks and rings, warmed up twice, then timed in 5 windows per build,
alternated parent / change; a package's figures pool the windows of its builds (two builds of ONE package differ by more than the
windows of a build do: ``instance_medians``).  ``within_parent_spread``: the change's median lies within the parent's min - max.
profiles/block_actor_ab.json holds three runs of this script (--builds 1, --builds 2, --builds 4 --only b64)."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = 5
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
DEV = "cuda:0"


def load(name, root):
    """The package under ``root`` as module ``name`` (its relative imports stay inside it)."""
    d = os.path.join(root, "sus-net_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def seeded(sn, dims, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return sn.MLP(dims).to(DEV).eval()


# ---- the workloads: each returns (run, units of work per run, unit name, better) ----
def train_loop(sn, batch=65536, steps=5001, bs=32):  # tools/train_loop_bench.py, variant (b)
    env = sn.BatchedFourRoomEnv(1, 2, 4, batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=14,
                                obs=sn.ObsConfig("flat", COMPS3), export_state=False, check_errors=False)
    imp, crew = sn.policy.reference_imposter_mlp(env, COMPS3, seed=3), sn.policy.reference_crew_mlp(env, COMPS3, seed=4)
    policy = sn.PolicyRollout(env, imp, crew, components=COMPS3, mask_dead=True)
    trainer = sn.DeviceDQNTeamTrainer(env, imp, crew, COMPS3, lr=1e-4, gamma=0.99, policy=policy)
    ring = sn.DeviceReplayBuffer(batch * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 8)
    sched = sn.ExponentialSchedule(1.0, 0.05, 1_000_000)
    tmp = tempfile.mkdtemp()

    def run():
        sn.train(env, sn.EpisodicMetricHandler(), steps, ring, policy, trainer, sched, tmp, train_step_interval=5, batch_size=bs, num_saves=1,
                 target_update_interval=10_000)
    return run, steps * batch, "transitions/s", "higher"


def dense_collect(sn, batch=65536, ticks=200, T=1, game="tagging", append=16):  # tools/dense_qnet_bench.py (2b), tools/window_bench.py (2)
    kw = dict(batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=9, export_state=False, check_errors=False)
    if game == "tagging":
        comps = COMPS3
        env = sn.BatchedFourRoomEnvWithTagging(1, 4, 5, obs=sn.ObsConfig("flat", comps), **kw)
    else:
        comps = COMPS3
        env = sn.BatchedFourRoomEnv(1, 3, 5, obs=sn.ObsConfig("flat", comps), **kw)
    env.reset()
    F = env.obs.shape[-1]
    imp = seeded(sn, [T * F, 256, 128, 64, 16, env.n_imposter_actions], 3)
    crew = seeded(sn, [T * F, 256, 128, 64, 16, env.n_crew_actions], 4)
    pol = sn.PolicyRollout(env, imp, crew, components=comps, dense=True, sequence_length=T)
    assert pol.dense_imposter is not None and pol.dense_crew is not None and pol.fused_imposter is None
    ring = sn.DeviceReplayBuffer(batch * 16, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)

    def run():
        ring.collect(env, pol, ticks, epsilon=0.1, mask_dead=True, ticks_per_append=append)
    return run, ticks, "us/tick", "lower"


def spatial_net(sn, env, Fn, n_actions, seed):  # tools/spatial_bench.py: the notebook's network
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = sn.SpatialDQN(input_image_size=env.n_rows, non_spatial_input_size=Fn, n_channels=[env.n_agents + 2, 5, 3], strides=[1, 1], paddings=[1, 1],
                          kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=64, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 16],
                          n_actions=n_actions)
    return m.to(env.device).eval()


def spatial_collect(sn, batch=65536, ticks=5, T=2):  # tools/spatial_collect_bench.py
    env = sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=9,
                                           obs=sn.ObsConfig("raw", dtype=torch.uint8), check_errors=False)
    feat = sn.GlobalFeaturizer(env)
    Fn = env._make_obs(feat.config, 1, rows=1)[2].shape[-1] + env.n_agents
    imp, crew = spatial_net(sn, env, Fn, env.n_imposter_actions, 3), spatial_net(sn, env, Fn, env.n_crew_actions, 4)
    pol = sn.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, mask_dead=True, kernels=True)
    assert pol.spatial_imposter is not None and pol.spatial_crew is not None
    ring = sn.DeviceReplayBuffer(batch * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    env.reset()

    def run():
        ring.collect(env, pol, ticks, epsilon=0.05, mask_dead=True, ticks_per_append=ticks)
    return run, ticks, "us/tick", "lower"


def fused_collect(sn, batch=65536, ticks=256, one_launch=True, append=64):  # bench.py's collect_into_replay_ring
    env = sn.BatchedFourRoomEnv(1, 2, 4, grid_size=14, batch=batch, device=DEV, rng="philox", seed=0, env_id_base=0, auto_reset=True,
                                export_state=False, check_errors=False, obs=sn.ObsConfig("flat", COMPS3))
    env.reset()
    pol = sn.PolicyRollout(env, sn.policy.reference_imposter_mlp(env, COMPS3, seed=0), None, components=COMPS3, epsilon=0.1, mask_dead=True)
    assert pol.fused_imposter is not None
    ring = sn.DeviceReplayBuffer(1 << 21, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=DEV)

    def run():
        ring.collect(env, pol, ticks, epsilon=0.1, ticks_per_append=append, one_launch_per_block=one_launch)
    return run, ticks * batch, "transitions/s", "higher"


def evaluate_fused(sn, batch=64, ticks=512, block=64):
    env = sn.BatchedFourRoomEnv(1, 2, 4, batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=14, obs=sn.ObsConfig("flat", COMPS3),
                                export_state=False, check_errors=False)
    imp = sn.policy.reference_imposter_mlp(env, COMPS3, seed=3)

    def run():
        sn.evaluate(env, imp, None, COMPS3, ticks, epsilon=0.1, block_ticks=block)
    return run, ticks, "us/tick", "lower"


def evaluate_dense(sn, batch=64, ticks=200, block=16, T=2):
    env = sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=9,
                                           obs=sn.ObsConfig("flat", ["onehot_pos"]), export_state=False, check_errors=False)
    env.reset()
    F = env.obs.shape[-1]
    imp, crew = seeded(sn, [T * F, 64, env.n_imposter_actions], 3), seeded(sn, [T * F, 64, env.n_crew_actions], 4)

    def run():
        sn.evaluate(env, imp, crew, ["onehot_pos"], ticks, epsilon=0.1, block_ticks=block, sequence_length=T)
    return run, ticks, "us/tick", "lower"


WORKLOADS = {
    # the tools' shapes (their defaults): bound by the device
    "train_loop_b65536_bs32_transitions_per_s": lambda sn: train_loop(sn),
    "dense_collect_tagging_1v4_b65536_us_per_tick": lambda sn: dense_collect(sn),
    "window_collect_base_1v3_T1_b65536_us_per_tick": lambda sn: dense_collect(sn, ticks=100, T=1, game="base"),
    "window_collect_base_1v3_T2_b65536_us_per_tick": lambda sn: dense_collect(sn, ticks=100, T=2, game="base"),
    "spatial_collect_T2_b65536_us_per_tick": lambda sn: spatial_collect(sn, T=2),
    "spatial_collect_T6_b65536_us_per_tick": lambda sn: spatial_collect(sn, T=6),
    "bench_py_collect_cfg5_b65536_transitions_per_s": lambda sn: fused_collect(sn),
    # the same loops at 64 envs: bound by the host, where a per-tick Python cost would show
    "train_loop_b64_bs32_transitions_per_s": lambda sn: train_loop(sn, batch=64, steps=2001),
    "fused_ticks_collect_b64_transitions_per_s": lambda sn: fused_collect(sn, batch=64, ticks=512, one_launch=False, append=16),
    "fused_block_of_5_collect_b64_transitions_per_s": lambda sn: fused_collect(sn, batch=64, ticks=500, append=5),
    "dense_collect_tagging_1v4_b64_us_per_tick": lambda sn: dense_collect(sn, batch=64, ticks=400),
    "window_collect_base_1v3_T2_b64_us_per_tick": lambda sn: dense_collect(sn, batch=64, ticks=400, T=2, game="base"),
    "spatial_collect_T2_b64_us_per_tick": lambda sn: spatial_collect(sn, batch=64, ticks=100, T=2),
    "evaluate_fused_b64_us_per_tick": lambda sn: evaluate_fused(sn),
    "evaluate_dense_T2_b64_us_per_tick": lambda sn: evaluate_dense(sn),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a directory that holds the other version's sus-net_amd/")
    ap.add_argument("--builds", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated substrings of workload names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_actor_ab_run.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "block_actor_ab needs the MI355X"
    if not os.path.exists(os.path.join(args.parent, "sus-net_amd", "libsusnet_hip.so")):
        os.environ.setdefault("SUSNET_LIB_PATH", os.path.join(ROOT, "sus-net_amd", "libsusnet_hip.so"))
    pkgs = {"parent": load("susnet_parent", os.path.abspath(args.parent)), "change": load("susnet_change", ROOT)}
    only = [o for o in args.only.split(",") if o]
    result = {"device": torch.cuda.get_device_name(0), "windows": WINDOWS, "builds": args.builds, "rows": {}}
    for name, make in WORKLOADS.items():
        if only and not any(o in name for o in only):
            continue
        runs, meta = {}, None
        for k in range(args.builds):
            for side, sn in pkgs.items():
                run, work, unit, better = make(sn)
                runs[(side, k)], meta = run, (work, unit, better)
        work, unit, better = meta
        for _ in range(2):
            for run in runs.values():
                run()
        windows = {key: [] for key in runs}
        for _ in range(WINDOWS):
            for key, run in runs.items():
                dt = timed(run)
                windows[key].append(work / dt if better == "higher" else dt * 1e6 / work)
        row = {"unit": unit, "better": better}
        for side in pkgs:
            v = [x for k in range(args.builds) for x in windows[(side, k)]]
            row[side] = {"median": statistics.median(v), "min": min(v), "max": max(v),
                         "instance_medians": [statistics.median(windows[(side, k)]) for k in range(args.builds)],
                         "windows": [windows[(side, k)] for k in range(args.builds)]}
        p, c = row["parent"], row["change"]
        row["change_over_parent"] = c["median"] / p["median"]
        row["within_parent_spread"] = p["min"] <= c["median"] <= p["max"]
        row["not_worse_than_parent_spread"] = c["median"] >= p["min"] if better == "higher" else c["median"] <= p["max"]
        result["rows"][name] = row
        print(name, json.dumps({side: [round(row[side][f], 3) for f in ("median", "min", "max")] for side in pkgs}),
              "ratio %.4f" % row["change_over_parent"], "within" if row["within_parent_spread"] else "OUTSIDE", flush=True)
        del runs
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:  # (after every workload: a run that is cut short keeps what it measured)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
