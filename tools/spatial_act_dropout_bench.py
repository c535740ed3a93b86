#!/usr/bin/env python3
"""What acting under dropout costs, on the network and game of notebooks/experiment.ipynb (tools/spatial_bench.py: tagging 1v4, 5 jobs,
9x9, GlobalFeaturizer, n_channels [7, 5, 3], three RNN layers of 64 with rnn_dropout 0.2, head [16, 16]) at T = 2 and T = 6:

  (1) one team's forward on the B * A rows of one tick: SpatialQNet(act_dropout_seed=...) on the module in training mode
      (susnet_spatial_forward_dropout: the plain convolution kernel + k_spatial_rnn_dropout) against the same object on the module in
      eval() (susnet_spatial_forward), same rows, same buffers;
  (2) the tick of DeviceReplayBuffer.collect with a WindowedPolicyRollout(kernels=True, act_dropout_seed=...), both teams' models in
      training mode, against the same policy class on the same models in eval mode -- each side on its own env of the same seed.

The two sides of each pair are warmed up, then timed REPEATS times in alternation with a device synchronise at the end of each window;
the JSON holds every repeat, the median and the min-max spread.

    python tools/spatial_act_dropout_bench.py [--batch 65536] [--calls 10] [--ticks 5] [--repeats 5] [--windows 2,6]
                                            [--out profiles/spatial_act_dropout_bench.json]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spatial_bench import alternate, notebook_network, sn, summary  # noqa: E402
from spatial_collect_bench import game  # noqa: E402

P, SEED = 0.2, 2


def dropout_network(env, Fn, n_actions, seed):
    """notebook_network's weights under rnn_dropout = 0.2 (dropout has no parameters), in training mode as a fresh module is."""
    m = notebook_network(env, Fn, n_actions, seed)
    m.rnn.model.dropout = P
    return m.train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--windows", default="2,6", help="the window lengths T, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_act_dropout_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spatial_act_dropout_bench needs the MI355X"
    B = args.batch
    result = {"batch": B, "calls": args.calls, "ticks": args.ticks, "repeats": args.repeats, "p": P, "device": torch.cuda.get_device_name(0), "rows": []}
    for T in (int(x) for x in args.windows.split(",")):
        envs = [game(B), game(B)]
        A = envs[0].n_agents
        feats = [sn.GlobalFeaturizer(e) for e in envs]
        Fn = envs[0]._make_obs(feats[0].config, 1, rows=1)[2].shape[-1] + A
        train_models = [dropout_network(envs[0], Fn, envs[0].n_imposter_actions, 3), dropout_network(envs[0], Fn, envs[0].n_crew_actions, 4)]
        eval_models = [copy.deepcopy(m).eval() for m in train_models]
        under = sn.WindowedPolicyRollout(envs[0], feats[0], *train_models, sequence_length=T, mask_dead=True, kernels=True, act_dropout_seed=SEED)
        plain = sn.WindowedPolicyRollout(envs[1], feats[1], *eval_models, sequence_length=T, mask_dead=True, kernels=True)
        assert under.spatial_crew.act_dropout_p() == P and plain.spatial_crew.act_dropout_p() == 0.0
        rings = [sn.DeviceReplayBuffer(B * args.ticks, e.flattened_state_size, T, A, e.n_imposters, device=e.device) for e in envs]
        for e in envs:
            e.reset()
        # (1) one team's forward on one tick's rows: the imposters' network on the first policy's feed, in both modes
        under.reset_window()
        under.q_rows()
        feed, qnet, model = under._feed, under.spatial_imposter, train_models[0]

        def forward_in(training):
            def run():
                model.train(training)
                for k in range(args.calls):
                    qnet.forward(feed.spatial, feed.non_spatial, A, net=2, offset=k)
            return run

        t = alternate({"dropout": forward_in(True), "eval": forward_in(False)}, args.repeats)
        model.train()
        row = {"T": T, "rows": B * A, "forward_us": {k: summary([x / args.calls * 1e6 for x in v]) for k, v in t.items()}}
        row["forward_dropout_over_eval"] = row["forward_us"]["dropout"]["median"] / row["forward_us"]["eval"]["median"]
        # (2) the collect tick
        collect = lambda i, policy: (lambda: rings[i].collect(envs[i], policy, args.ticks, epsilon=0.05, mask_dead=True, ticks_per_append=args.ticks))
        t = alternate({"dropout": collect(0, under), "eval": collect(1, plain)}, args.repeats)
        row["collect_tick_us"] = {k: summary([x / args.ticks * 1e6 for x in v]) for k, v in t.items()}
        row["collect_dropout_over_eval"] = row["collect_tick_us"]["dropout"]["median"] / row["collect_tick_us"]["eval"]["median"]
        result["rows"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b["median"], 1) for a, b in v.items()}) for k, v in row.items()}), flush=True)
        del envs, feats, under, plain, rings, feed, qnet
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (after every window length: a run that is cut short keeps what it measured)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
