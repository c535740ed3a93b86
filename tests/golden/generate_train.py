#!/usr/bin/env python3
"""Golden vectors of the reference trainer's LEARNING step (container only).

    python tests/golden/generate_train.py        # rewrites tests/golden/model_train_*.npz

Runs the UNMODIFIED `DQNTeamTrainer.train_step` of src/train.py (50-149) with `torch.optim.Adam` (OptimizerType.build, train.py:24-38) on
replay batches drawn from a reference `ReplayBuffer`, K steps per configuration.  src/train.py imports pygame, ipywidgets, IPython.display,
matplotlib and src.visualize (a module this Python cannot parse); minimal stand-ins for those five are installed below -- none of them is
touched by `train_step`.  Stored (data only): the ring rows, their FlatFeaturizer rows as uint8 (the reference featurizer's output), the
sampled indices of every step, the initial parameters of both teams (the targets are copies of them, train.py:306-307, and train_step
never syncs them), the losses of every step, Adam's exp_avg after the first step, and the parameters, exp_avg, exp_avg_sq and step
counts after the last one.  The package's torch path (tests/test_train_host.py) and HIP path (tests/test_gpu_train.py) are compared with them.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refshim  # noqa: E402

_refshim.install()
import torch  # noqa: E402


def _stand_ins():
    """Empty modules for what src/train.py imports but train_step never uses."""
    for name in ("pygame", "ipywidgets", "IPython", "IPython.display", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["IPython"].display = sys.modules["IPython.display"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    vis = types.ModuleType("src.visualize")
    vis.AmongUsVisualizer = type("AmongUsVisualizer", (), {})
    sys.modules["src.visualize"] = vis


_stand_ins()
from generate_golden import GRID14, make_env  # noqa: E402
from src.features import component as comp  # noqa: E402
from src.features.model_ready import FlatFeaturizer  # noqa: E402
from src.models.dqn import MLP  # noqa: E402
from src.replay_memory import Batch, ReplayBuffer  # noqa: E402
from src.train import DQNTeamTrainer, OptimizerType  # noqa: E402

PARTS = {"onehot_pos": comp.OneHotAgentPositionFeaturizer, "coord_pos": comp.CoordinateAgentPositionsFeaturizer,
         "alive_crew": comp.AliveCrewFeaturizer, "closest_crew": comp.ClosestAliveCrewFeaturizer}
GRID9_WALLS = None  # the reference ImposterTrainingGround's own four-room map (include_walls=True)


def ring_from_collect(name):
    """The ring of a reference collection run already pinned in tests/golden (collect_*.npz, generate_collect.py): episodes that end by kills."""
    d = np.load(os.path.join(HERE, f"collect_{name}.npz"))
    return {k: d[k] for k in ("states", "next_states", "actions", "rewards", "dones", "imposters")}


def ring_from_populate(spec, n_rows, seed):
    env = make_env(spec)
    buf = ReplayBuffer(n_rows, env.flattened_state_size, 1, env.n_agents, env.n_imposters)
    np.random.seed(seed)
    buf.populate(env, n_rows)
    n = buf.size
    return {"states": buf.states[:n].numpy(), "next_states": buf.next_states[:n].numpy(), "actions": buf.actions[:n].numpy(),
            "rewards": buf.rewards[:n].numpy(), "dones": buf.dones[:n].numpy().astype(np.uint8), "imposters": buf.imposters[:n].numpy()}


def run(name, spec, ring, components, hidden, train_imposter, train_crew, gamma, lr, batch_sizes, seed):
    env = make_env(spec)
    feat = FlatFeaturizer(env, comp.CompositeFeaturizer([PARTS[c](env) for c in components]))
    F = int(feat.featurized_shape[1][0])
    torch.manual_seed(seed)
    imp = MLP([F, *hidden, env.n_imposter_actions])
    crew = MLP([F, *hidden, env.n_crew_actions])
    imp_t, crew_t = imp.create_copy(), crew.create_copy()  # train.py:306-307
    init = {"imposter::" + k: v.detach().numpy().copy() for k, v in imp.state_dict().items()}
    init.update({"crew::" + k: v.detach().numpy().copy() for k, v in crew.state_dict().items()})
    opt_i = OptimizerType.build("adam", imp, lr) if train_imposter else None
    opt_c = OptimizerType.build("adam", crew, lr) if train_crew else None
    trainer = DQNTeamTrainer(opt_i, opt_c, gamma)
    T = {"states": torch.tensor(ring["states"], dtype=torch.float32), "next_states": torch.tensor(ring["next_states"], dtype=torch.float32),
         "actions": torch.tensor(ring["actions"], dtype=torch.int64), "rewards": torch.tensor(ring["rewards"], dtype=torch.float32),
         "dones": torch.tensor(ring["dones"], dtype=torch.bool).reshape(-1, 1), "imposters": torch.tensor(ring["imposters"], dtype=torch.int16)}
    M = T["states"].shape[0]
    # the featurized rows of the whole ring (what the CPU test feeds the torch path)
    feat.fit(T["states"])
    f_states = feat.generate_featurized_states()[0][1].detach().numpy()
    feat.fit(T["next_states"])
    f_next = feat.generate_featurized_states()[0][1].detach().numpy()
    g = torch.Generator().manual_seed(seed)
    idx_all, losses, first = [], [], {}
    for k, bs in enumerate(batch_sizes):
        idx = torch.randint(0, M, (bs,), generator=g)  # ReplayBuffer.sample (replay_memory.py:89)
        batch = Batch(states=T["states"][idx], actions=T["actions"][idx], rewards=T["rewards"][idx], next_states=T["next_states"][idx],
                      imposters=T["imposters"][idx], dones=T["dones"][idx])
        losses.append(trainer.train_step(batch, feat, imp, imp_t, crew, crew_t))
        idx_all.append(idx.numpy())
        if k == 0:
            for team, opt, model in (("imposter", opt_i, imp), ("crew", opt_c, crew)):
                if opt is None:
                    continue
                names = dict((id(p), n) for n, p in model.named_parameters())
                for p in model.parameters():
                    st = opt.state.get(p)
                    if st:
                        first[f"first_exp_avg::{team}::{names[id(p)]}"] = st["exp_avg"].numpy().copy()
    final = {}
    for team, opt, model in (("imposter", opt_i, imp), ("crew", opt_c, crew)):
        for n, p in model.named_parameters():
            final[f"final::{team}::{n}"] = p.detach().numpy().copy()
            st = opt.state.get(p) if opt is not None else None
            final[f"final_exp_avg::{team}::{n}"] = st["exp_avg"].numpy().copy() if st else np.zeros(p.shape, np.float32)
            final[f"final_exp_avg_sq::{team}::{n}"] = st["exp_avg_sq"].numpy().copy() if st else np.zeros(p.shape, np.float32)
            final[f"final_step::{team}::{n}"] = np.array(float(st["step"]) if st else 0.0, np.float32)
    meta = dict(spec, components=components, hidden=list(hidden), train_imposter=train_imposter, train_crew=train_crew, gamma=gamma, lr=lr,
                batch_sizes=list(batch_sizes), seed=seed, F=F, n_agents=int(env.n_agents), n_imposters=int(env.n_imposters),
                state_size=int(env.flattened_state_size), imposter_dims=[F, *hidden, int(env.n_imposter_actions)],
                crew_dims=[F, *hidden, int(env.n_crew_actions)], done_rows=int(ring["dones"].sum()))
    out = os.path.join(HERE, f"model_train_{name}.npz")
    np.savez_compressed(out, meta=json.dumps(meta), **{"ring::" + k: v for k, v in ring.items()}, feat_states=f_states.astype(np.uint8).reshape(M, -1),
                        feat_next_states=f_next.astype(np.uint8).reshape(M, -1), indices=np.concatenate(idx_all).astype(np.int32),
                        losses=np.array(losses, dtype=np.float64), **{"init::" + k: v for k, v in init.items()}, **first, **final)
    print(name, "rows", M, "done rows", meta["done_rows"], "losses[0]", losses[0], os.path.getsize(out), "bytes")


def main():
    itg = {"class": "itg", "kwargs": {"n_crew": 1, "n_jobs": 0, "kill_reward": -3, "sabotage_reward": 0, "end_of_game_reward": 0,
                                      "time_step_reward": 0, "include_walls": False}}
    itg_w = {"class": "itg", "kwargs": dict(itg["kwargs"], include_walls=True)}
    base14 = {"class": "base", "kwargs": dict(n_imposters=1, n_crew=2, n_jobs=4, shuffle_imposter_index=True, max_time_steps=60),
              "grid": GRID14.astype(int).tolist()}
    K = 20
    # the notebook setup: 1v1 no walls, onehot_pos, imposter trained, random crew, gamma 0.9, batch 8 (experiment_1v1.ipynb cell 1)
    run("itg_1v1_onehot", itg, ring_from_collect("itg_1v1_nowalls_kills_t1"), ["onehot_pos"], (16, 16, 8, 8), True, False, 0.9, 1e-2, [8] * K, 11)
    # the wall map, coord_pos
    run("itg_1v1_walls_coord", itg_w, ring_from_populate(itg_w, 400, 12), ["coord_pos"], (16, 16, 8, 8), True, False, 0.9, 1e-2, [8] * K, 12)
    # 1v2 14x14, shuffled imposter index, both teams: batch 32 with a few tiny batches (skipped (agent, team) updates)
    sizes = [32] * K
    sizes[3], sizes[7], sizes[12] = 1, 2, 3
    run("base14_1v2_j4", base14, ring_from_populate(base14, 400, 13), ["onehot_pos", "alive_crew", "closest_crew"], (16, 16, 8, 8), True, True, 0.9,
        1e-2, sizes, 13)


if __name__ == "__main__":
    main()
