"""What partial observability costs: ``susnet_featurize`` in the modes ``persp`` / ``persp_room`` / ``persp_room_mask`` and the
``WindowedPolicyRollout(kernels=True)`` collect tick with plain and with partially observable Perspective features, at 65 536 envs of the
notebook's game (tagging 1v4, 5 jobs, 9x9).  The baseline is the PARENT commit's ``persp`` featurize in the same process on the same
machine: ``--parent DIR`` holds the parent's package with its own built library, e.g.

    mkdir /tmp/parent && git archive <commit> | tar -x -C /tmp/parent && python /tmp/parent/sus-net_amd/build_hip.py
    python tools/persp_room_bench.py --parent /tmp/parent [--out profiles/persp_room_bench.json]

Every figure is the median of 5 windows, the variants alternated window by window (min - max recorded).  A featurize window is ``--reps``
launches into buffers made once (float32 outputs, uint8 rows: what the acting path and the trainer feed); a tick window is one
``DeviceReplayBuffer.collect`` of 5 ticks.  ``expected`` is the parent's ``persp`` time scaled by the bytes written; the masked form
writes the same bytes (+ 1 / (A + 2) with the mask channel) and adds one AND per element."""
from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS, DEV = 5, "cuda:0"


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


def game(sn, batch):
    return sn.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=1, auto_reset=True, grid_size=9,
                                            obs=sn.ObsConfig("raw", dtype=torch.uint8), check_errors=False)


def featurize_run(sn, env, rows, mode, reps):
    """-> (run, bytes written per launch): ``reps`` launches of ``susnet_featurize`` over ``rows`` into buffers made once."""
    L = sn._lib
    spec, o1, o2 = env._make_obs(sn.ObsConfig(mode), 1, rows=rows.shape[0])
    dtype = env._ROW_DTYPES[rows.dtype]

    def run():
        for _ in range(reps):
            L.check(env.lib.susnet_featurize(env._h, rows.data_ptr(), dtype, rows.shape[0], C.byref(spec), env._stream()))
    return run, o1.numel() * o1.element_size() + o2.numel() * o2.element_size(), (o1, o2)


def spatial_net(sn, env, channels, Fn, n_actions, seed):  # tools/spatial_bench.py: the notebook's network
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = sn.SpatialDQN(input_image_size=env.n_rows, non_spatial_input_size=Fn, n_channels=[channels, 5, 3], strides=[1, 1], paddings=[1, 1],
                          kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=64, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 16],
                          n_actions=n_actions)
    return m.to(env.device).eval()


def collect_run(sn, batch, feat_kw, ticks=5, T=2):
    env = game(sn, batch)
    feat = sn.PerspectiveFeaturizer(env, **feat_kw)
    _, planes, non = env._make_obs(feat.config, 1, rows=1)
    imp = spatial_net(sn, env, planes.shape[-3], non.shape[-1], env.n_imposter_actions, 3)
    crew = spatial_net(sn, env, planes.shape[-3], non.shape[-1], env.n_crew_actions, 4)
    pol = sn.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, mask_dead=True, kernels=True)
    assert pol.spatial_imposter is not None and pol.spatial_crew is not None
    ring = sn.DeviceReplayBuffer(batch * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    env.reset()

    def run():
        ring.collect(env, pol, ticks, epsilon=0.05, mask_dead=True, ticks_per_append=ticks)
    return run, ticks


def measure(variants, scale):
    """variants: {name: run}; -> {name: {median, min, max}} in the unit ``scale`` converts seconds to; 2 warm-up rounds, then WINDOWS
    rounds with the variants alternated."""
    for _ in range(2):
        for run in variants.values():
            timed(run)
    samples = {name: [] for name in variants}
    for _ in range(WINDOWS):
        for name, run in variants.items():
            samples[name].append(timed(run) * scale[name])
    return {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "persp_room_bench.json"))
    args = ap.parse_args()
    new, parent = load("susnet_new", ROOT), load("susnet_parent", args.parent)
    assert not hasattr(parent._lib, "OBS_PERSP_ROOM"), "--parent must hold the commit before the room modes"
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "game": "tagging 1v4, 5 jobs, 9x9", "windows": WINDOWS,
              "featurize_reps_per_window": args.reps, "featurize_us": {}, "collect_tick_us": {}}
    env_new, env_parent = game(new, args.batch), game(parent, args.batch)
    env_new.reset()
    for T in (2, 6):
        rows = env_new.observe(new.ObsConfig("raw", dtype=torch.uint8)).repeat(T, 1).contiguous()  # [batch * T, S] valid rows
        runs, nbytes, keep = {}, {}, []
        for name, (sn, env, mode) in {"parent_persp": (parent, env_parent, "persp"), "persp": (new, env_new, "persp"),
                                      "persp_room": (new, env_new, "persp_room"), "persp_room_mask": (new, env_new, "persp_room_mask")}.items():
            runs[name], nbytes[name], bufs = featurize_run(sn, env, rows, mode, args.reps)
            keep.append(bufs)
        got = measure(runs, {name: 1e6 / args.reps for name in runs})
        base = got["parent_persp"]
        for name, g in got.items():
            g["bytes_written"] = nbytes[name]
            g["GB_per_s"] = nbytes[name] / g["median"] / 1e3
            g["expected_us"] = base["median"] * nbytes[name] / nbytes["parent_persp"]
            g["over_expected"] = g["median"] / g["expected_us"]
        got["parent_spread"] = (base["max"] - base["min"]) / base["median"]
        result["featurize_us"][f"T={T}"] = got
        print(f"T={T}", json.dumps({k: (round(v["median"], 1), round(v["over_expected"], 3)) for k, v in got.items() if isinstance(v, dict)}))
        del runs, keep
        torch.cuda.empty_cache()
    ticks = {}
    runs = {"persp": collect_run(new, args.batch, {}), "persp_room": collect_run(new, args.batch, dict(partially_observable=True, add_obs_mask_feature=False)),
            "persp_room_mask": collect_run(new, args.batch, dict(partially_observable=True))}
    ticks = measure({k: r for k, (r, _) in runs.items()}, {k: 1e6 / n for k, (_, n) in runs.items()})
    for name, g in ticks.items():
        g["over_plain"] = g["median"] / ticks["persp"]["median"]
    result["collect_tick_us"] = ticks
    print("collect tick", json.dumps({k: (round(v["median"], 1), round(v["over_plain"], 3)) for k, v in ticks.items()}))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
