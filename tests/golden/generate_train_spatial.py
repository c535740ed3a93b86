#!/usr/bin/env python3
"""Golden vectors of the reference trainer's learning step on its default model, the SpatialDQN (container only).

    python tests/golden/generate_train_spatial.py        # rewrites tests/golden/spatial_train/train_*.npz

The UNMODIFIED `DQNTeamTrainer.train_step` (src/train.py:50-149) with `torch.optim.Adam`, the UNMODIFIED `SpatialDQN`
(src/models/dqn.py:205-301) and the reference's own `GlobalFeaturizer` / `PerspectiveFeaturizer` on a reference `ReplayBuffer` of windows
(`populate`, replay_memory.py:96-140).  On the BASE game: the reference's GlobalFeaturizer raises on the tagging game (generate_spatial.py
has the lines).  As in generate_train_dense.py, `dones` is set on every 8th ring row BEFORE the reference trains on it (random play ends too
few episodes in so few rows; recorded in `meta`: the input is ours, every output is the reference's).  Stored as data: the ring, the
reference featurizers' tensors of the whole ring (what a CPU test feeds the package's torch path), the sampled indices, the losses of
every step, the parameters by state_dict key at the start and after every step, Adam's exp_avg after the first step and its step counts.
The files go to a directory of their own, spatial_train/, as generate_train_dense.py's go to dense/: tests/golden/spatial/ holds the
forward's fixtures and nothing else (tests/test_spatial_abi.py globs it and pins its contents).
tests/test_spatial_train_host.py (the package's torch path) and tests/test_gpu_spatial_train.py (susnet_spatial_train_step) are compared
with them.
"""
from __future__ import annotations

import json
import os

import numpy as np

import generate_train as gt  # noqa: E402  (installs the import shims)
import torch  # noqa: E402
from generate_golden import GRID14, make_env  # noqa: E402
from src.features.model_ready import GlobalFeaturizer, PerspectiveFeaturizer  # noqa: E402
from src.models.dqn import SpatialDQN  # noqa: E402
from src.replay_memory import Batch, ReplayBuffer  # noqa: E402
from src.train import DQNTeamTrainer, OptimizerType  # noqa: E402

OUT = os.path.join(gt.HERE, "spatial_train")
ROWS, DONE_EVERY = 96, 8
TEAMS = ("imposter", "crew")


def small_whole(a, what):
    out = np.asarray(a).astype(np.uint8)
    assert np.array_equal(out.astype(np.float64), np.asarray(a, dtype=np.float64)), f"{what}: small whole numbers"
    return out


def run(name, spec, featurizer_cls, T, cfg_of, gamma, lr, batch_sizes, seed):
    env = make_env(spec)
    buf = ReplayBuffer(ROWS, env.flattened_state_size, T, env.n_agents, env.n_imposters)
    np.random.seed(seed)
    buf.populate(env, ROWS)
    assert buf.size == ROWS
    natural = int(buf.dones.sum())
    buf.dones.view(-1)[::DONE_EVERY] = True
    feat = featurizer_cls(env)
    views = {}
    for key, states in (("", buf.states), ("next_", buf.next_states)):
        feat.fit(states)
        v = feat.generate_featurized_states()
        views[key + "spatial"] = torch.stack([x[0].detach().float() for x in v], dim=2).numpy()          # [M, T, A, C, N, N]
        views[key + "non_spatial"] = torch.stack([x[1].detach().float() for x in v], dim=2).numpy()      # [M, T, A, Fn]
    sp = views["spatial"]
    cfg = cfg_of(int(sp.shape[3]), int(sp.shape[-1]), int(views["non_spatial"].shape[-1]))
    models, targets, opts = [], [], []
    for team, n_actions, mseed in ((TEAMS[0], env.n_imposter_actions, seed + 100), (TEAMS[1], env.n_crew_actions, seed + 200)):
        torch.manual_seed(mseed)
        m = SpatialDQN(**dict(cfg, n_actions=int(n_actions)))
        with torch.no_grad():
            for i, mod in enumerate(x for x in m.modules() if isinstance(x, torch.nn.PReLU)):
                mod.weight.fill_((0.1, 0.3, 0.5)[i])
        models.append(m), targets.append(m.create_copy()), opts.append(OptimizerType.build("adam", m, lr))
    arrays = {f"init::{team}::{k}": v.detach().numpy().copy() for team, m in zip(TEAMS, models) for k, v in m.state_dict().items()}
    trainer = DQNTeamTrainer(opts[0], opts[1], gamma)
    g = torch.Generator().manual_seed(seed)
    idx_all, losses = [], []
    for k, bs in enumerate(batch_sizes):
        idx = torch.randint(0, ROWS, (bs,), generator=g)  # ReplayBuffer.sample (replay_memory.py:89)
        batch = Batch(states=buf.states[idx], actions=buf.actions[idx], rewards=buf.rewards[idx], next_states=buf.next_states[idx],
                      imposters=buf.imposters[idx], dones=buf.dones[idx])
        losses.append(trainer.train_step(batch, feat, models[0], targets[0], models[1], targets[1]))
        idx_all.append(idx.numpy())
        for team, m, opt in zip(TEAMS, models, opts):
            for n, p in m.named_parameters():
                arrays[f"step{k}::{team}::{n}"] = p.detach().numpy().copy()
                st = opt.state.get(p)
                if k == 0 and st:
                    arrays[f"first_exp_avg::{team}::{n}"] = st["exp_avg"].numpy().copy()
    steps = {team: float(next(iter(opt.state.values()))["step"]) for team, opt in zip(TEAMS, opts)}
    meta = dict(spec, featurizer=featurizer_cls.__name__, T=T, seed=seed, config=cfg, gamma=gamma, lr=lr, batch_sizes=list(batch_sizes),
                n_agents=int(env.n_agents), n_imposters=int(env.n_imposters), n_jobs=int(env.n_jobs), state_size=int(env.flattened_state_size),
                n_actions={TEAMS[0]: int(env.n_imposter_actions), TEAMS[1]: int(env.n_crew_actions)}, grid=env.grid.astype(int).tolist(),
                dones_set_every=DONE_EVERY, done_rows_from_play=natural, done_rows=int(buf.dones.sum()), final_step=steps)
    shared = featurizer_cls is GlobalFeaturizer  # every agent's view holds the same planes: stored once
    for key in ("spatial", "next_spatial"):
        v = small_whole(views[key], key)
        if shared:
            assert all(np.array_equal(v[:, :, 0], v[:, :, i]) for i in range(v.shape[2]))
            v = v[:, :, 0]
        arrays[key] = v
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"train_{name}.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), non_spatial=views["non_spatial"], next_non_spatial=views["next_non_spatial"],
                        **{"ring::states": small_whole(buf.states.numpy(), "states"), "ring::next_states": small_whole(buf.next_states.numpy(), "states"),
                           "ring::actions": buf.actions.numpy().astype(np.int8), "ring::rewards": buf.rewards.numpy(),
                           "ring::dones": buf.dones.numpy().astype(np.uint8), "ring::imposters": buf.imposters.numpy()},
                        indices=np.concatenate(idx_all).astype(np.int32), losses=np.array(losses, dtype=np.float64), **arrays)
    print(name, "planes", tuple(sp.shape), "done rows", meta["done_rows"], "steps", steps, "losses[0]", losses[0], os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


def main():
    # Global featurizer, T = 2: the notebook's game (1v4, 5 jobs, 9x9) with a narrow network of its shape (k = 3, the repeated last layer,
    # two RNN layers) so that the parameters after every step fit the size limit
    run("global_t2", dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=4, n_jobs=5, max_time_steps=40)), GlobalFeaturizer, 2,
        lambda C, N, Fn: dict(input_image_size=N, non_spatial_input_size=Fn, n_channels=[C, 4, 2], strides=[1, 1], paddings=[1, 1], kernel_size=[3, 3],
                              dilations=[1, 1], rnn_layers=2, rnn_hidden_dim=12, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 8]),
        0.9, 1e-2, [32, 1, 32, 7], 41)
    # Perspective featurizer, T = 3: 1v2, 4 jobs, 14x14 (generate_spatial.py's second game), a stride-2 first layer
    run("perspective_t3", dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=2, n_jobs=4, max_time_steps=40), grid=GRID14.astype(int).tolist()),
        PerspectiveFeaturizer, 3,
        lambda C, N, Fn: dict(input_image_size=N, non_spatial_input_size=Fn, n_channels=[C, 4, 2], strides=[2, 1], paddings=[1, 1], kernel_size=[3, 3],
                              dilations=[1, 1], rnn_layers=1, rnn_hidden_dim=12, rnn_dropout=0.0, mlp_hidden_layer_dims=[10]),
        0.9, 1e-2, [32, 32, 1, 9], 42)


if __name__ == "__main__":
    main()
