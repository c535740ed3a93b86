"""Microseconds per train step of a SpatialDQN trainer on its two paths: the spatial HIP step (susnet_spatial_train_step,
DeviceDQNTeamTrainer(spatial=True)) against the torch path (torch_train_step), both teams trained, on the two networks of
tests/golden/generate_spatial.py -- the notebook's (base 1v4, 5 jobs, 9x9, GlobalFeaturizer, T = 6, channels [7, 5, 3] with the repeated
last layer, k = 3, three RNN layers of 64, head [64, 16, 16, n]) and the Perspective one (base 1v2, 4 jobs, 14x14, T = 3, [5, 6, 8], one RNN
layer of 16, head [16, 12, n]).

Method: warm both sides up, then alternate them, 5 windows of --steps steps each, every window timed with device
events around work that ends in a synchronise; reported per side: the median window with (min - max).  Writes the JSON to --out (default
profiles/spatial_train_bench.json) and prints it as one line."""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
DEV = "cuda:0"
WINDOWS = 5


def game(name, batch):
    """-> (env, featurizer class, T, SpatialDQN config without n_actions)"""
    kw = dict(batch=batch, device=DEV, rng="philox", auto_reset=True, check_errors=False, shuffle_imposter_index=True)
    if name == "notebook_global_t6":
        env = pkg.BatchedFourRoomEnv(1, 4, 5, seed=3, grid_size=9, **kw)
        return env, pkg.GlobalFeaturizer, 6, dict(n_channels=[5, 3], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1], rnn_layers=3,
                                                  rnn_hidden_dim=64, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 16])
    assert name == "perspective_t3"
    env = pkg.BatchedFourRoomEnv(1, 2, 4, seed=5, grid_size=14, **kw)
    return env, pkg.PerspectiveFeaturizer, 3, dict(n_channels=[6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1], rnn_layers=1,
                                                   rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[12])


def models(env, Fz, cfg):
    _, planes, non = env._make_obs(Fz(env).config, 1, rows=1)
    Fn = non.shape[-1] + (env.n_agents if Fz is pkg.GlobalFeaturizer else 0)
    cfg = dict(cfg, input_image_size=planes.shape[-1], non_spatial_input_size=Fn, n_channels=[planes.shape[-3]] + cfg["n_channels"])
    out = []
    for seed, n_actions in ((3, env.n_imposter_actions), (4, env.n_crew_actions)):
        torch.manual_seed(seed)
        out.append(pkg.SpatialDQN(**cfg, n_actions=n_actions))
    return out


def window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps * 1e3


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="32,4096")
    ap.add_argument("--games", default="notebook_global_t6,perspective_t3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_train_bench.json"))
    args = ap.parse_args()
    out = {"unit": "us_per_train_step", "device": torch.cuda.get_device_name(0),
           "method": f"warm-up {args.warmup}, sides alternated, {WINDOWS} windows of {args.steps} steps timed with device events: median (min, max)",
           "games": {}}
    for name in args.games.split(","):
        env, Fz, T, cfg = game(name, 1024)
        ring = pkg.DeviceReplayBuffer(1024 * 16, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
        ring.populate_fused(env, 16)
        imp, crew = models(env, Fz, cfg)
        spatial = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], 1e-4, 0.9, featurizer=Fz(env), spatial=True)
        other = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(crew), [], 1e-4, 0.9, featurizer=Fz(env))
        assert spatial.uses_spatial(ring) and not other.uses_spatial(ring)
        rows = {}
        for n in [int(x) for x in args.sizes.split(",")]:
            idx = torch.randint(0, ring.size, (n,), device=DEV)
            r = alternate({"spatial": lambda: spatial.train_step_on_indices(ring, idx), "torch": lambda: other.train_step_on_indices(ring, idx)},
                          args.steps, args.warmup)
            r["spatial_speedup"] = round(r["torch"]["median"] / r["spatial"]["median"], 2)
            rows[str(n)] = r
            print(name, n, json.dumps(r), flush=True)
        out["games"][name] = {"agents": env.n_agents, "featurizer": Fz.__name__, "T": T, "teams_trained": 2, "config": cfg,
                              "launches_per_step": 1 + 4 * env.n_agents * 2, "parameters": [int(f.numel()) for f in spatial.flat], "sizes": rows}
        del env, ring, spatial, other
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
