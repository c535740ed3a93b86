#!/usr/bin/env python3
"""The feature-window kernel (susnet_window_push) measured, at n = 65 536 rows:

  (1) the push alone for (T, F) = (2, 88), (2, 324), (4, 88), (8, 128): microseconds per call and the bytes it moves per second --
      2 T F 4 bytes per row (the window read and written once; of it F 4 bytes come from `fresh` instead of `src`) plus the two flag
      bytes -- as a fraction of the HBM peak (8.0 TB/s), beside two comparisons timed in the same run, in alternation: a device-to-device
      `copy_` of the window's byte count (the same read + write traffic with no flags and no ragged rows), and the torch restatement
      `torch.where(ended, fresh.repeat(1, T), torch.cat([src[:, F:], fresh], 1))`;
  (2) the windowed dense collect tick (DeviceReplayBuffer.collect with PolicyRollout(dense=True, sequence_length=2)) against the T = 1
      dense collect tick on the same game, in env-steps/s: what the window costs end to end (a wider first layer + the push).

Every set is warmed up, then timed REPEATS times in alternation with a device synchronise at the end of each window; the JSON holds every
repeat, the median and the min-max spread.

    python tools/window_bench.py [--rows 65536] [--calls 200] [--ticks 100] [--repeats 5] [--out profiles/window_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
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

HBM_PEAK = 8.0e12  # bytes/s, the part's specification
SHAPES = [(2, 88), (2, 324), (4, 88), (8, 128)]
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]


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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "window_bench needs the MI355X"
    n, dev = args.rows, "cuda:0"
    result = {"rows": n, "calls": args.calls, "ticks": args.ticks, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "hbm_peak_bytes_per_s": HBM_PEAK, "push": [], "collect_tick": None}
    L = sn._lib
    env = sn.BatchedFourRoomEnv(1, 3, 5, batch=64, device=dev, rng="philox", seed=1, auto_reset=True, grid_size=9)  # (the handle only)

    for T, F in SHAPES:
        W = T * F
        src, dst = torch.rand(n, W, device=dev), torch.empty(n, W, device=dev)
        fresh = torch.rand(n, F, device=dev)
        done = torch.rand(n, device=dev) < 0.05
        trunc = torch.rand(n, device=dev) < 0.05
        io = L.WindowIO()
        io.fresh, io.src, io.dst, io.done, io.truncated = fresh.data_ptr(), src.data_ptr(), dst.data_ptr(), done.data_ptr(), trunc.data_ptr()
        io.T, io.F, io.n = T, F, n
        stream = env._stream()

        def push_calls():
            for _ in range(args.calls):
                L.check(env.lib.susnet_window_push(env._h, C.byref(io), stream))

        def copy_calls():
            for _ in range(args.calls):
                dst.copy_(src)

        def torch_calls():
            for _ in range(args.calls):
                torch.where((done | trunc).view(n, 1), fresh.repeat(1, T), torch.cat([src[:, F:], fresh], 1))

        push_calls()
        torch.cuda.synchronize()
        want = sn.policy.window_push_reference(src, fresh, done, trunc)
        assert torch.equal(dst.view(torch.int32), want.view(torch.int32)), "the timed kernel computes the restatement"
        t = alternate({"window_push": push_calls, "d2d_copy": copy_calls, "torch_restatement": torch_calls}, args.repeats)
        moved = n * (2 * W * 4 + 2)
        row = {"T": T, "F": F, "rows": n, "bytes_moved": moved}
        for k, ts in t.items():
            row[k + "_us_per_call"] = summary([1e6 * x / args.calls for x in ts])
        push_s = row["window_push_us_per_call"]["median"] * 1e-6
        row["window_push_bytes_per_s"] = moved / push_s
        row["window_push_fraction_of_hbm_peak"] = moved / push_s / HBM_PEAK
        row["push_over_copy"] = row["window_push_us_per_call"]["median"] / row["d2d_copy_us_per_call"]["median"]
        row["torch_over_push"] = row["torch_restatement_us_per_call"]["median"] / row["window_push_us_per_call"]["median"]
        result["push"].append(row)
        print(json.dumps(row), flush=True)
        del src, dst, fresh

    # (2) collect: T = 2 against T = 1 on base 1v3 9x9 5 jobs, both teams by the reference architecture on the dense kernel
    B = n
    runs, dims_of = {}, {}
    for T in (1, 2):
        e = sn.BatchedFourRoomEnv(1, 3, 5, batch=B, device=dev, rng="philox", seed=1, auto_reset=True, grid_size=9, obs=sn.ObsConfig("flat", COMPS3),
                                  export_state=False, check_errors=False)
        e.reset()
        Fe = e.obs.shape[-1]
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(3)
            imp = sn.MLP([T * Fe, 256, 128, 64, 16, e.n_imposter_actions]).to(dev).eval()
            crew = sn.MLP([T * Fe, 256, 128, 64, 16, e.n_crew_actions]).to(dev).eval()
        pol = sn.PolicyRollout(e, imp, crew, components=COMPS3, dense=True, sequence_length=T)
        assert pol.dense_imposter is not None and pol.dense_crew is not None and pol.fused_imposter is None
        ring = sn.DeviceReplayBuffer(B * 16, e.flattened_state_size, T, e.n_agents, e.n_imposters, device=e.device)
        dims_of[T] = pol.dense_imposter.dims

        def collect_run(ring=ring, e=e, pol=pol):
            ring.collect(e, pol, args.ticks, epsilon=0.1, mask_dead=True, ticks_per_append=16)

        runs[f"T{T}"] = collect_run
    t = alternate(runs, args.repeats)
    row = {"game": "base_1v3_9x9_j5", "batch": B, "ticks_per_append": 16, "imposter_dims": dims_of}
    for k, ts in t.items():
        row[k + "_collect_env_steps_per_s"] = summary([args.ticks * B / x for x in ts])
        row[k + "_collect_us_per_tick"] = summary([1e6 * x / args.ticks for x in ts])
    row["T2_over_T1_time"] = row["T2_collect_us_per_tick"]["median"] / row["T1_collect_us_per_tick"]["median"]
    result["collect_tick"] = row
    print(json.dumps(row), flush=True)

    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
