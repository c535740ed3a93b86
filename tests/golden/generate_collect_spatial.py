#!/usr/bin/env python3
"""Golden vectors of the reference trainer's COLLECTION loop with its default model, SpatialDQN (container only).

    python tests/golden/generate_collect_spatial.py        # rewrites tests/golden/spatial_collect/*.npz

`run_experiment` defaults both teams to `ModelType.SPATIAL_DQN` at `sequence_length=2` (src/train.py:152-176).  As in
generate_collect_window.py, `src/train.py` cannot be imported here, so its acting-and-collecting loop -- train.py:316-322, 345-399 and
419-449 -- is restated around the UNMODIFIED reference objects it drives: the env, the `GlobalFeaturizer` / `PerspectiveFeaturizer`, the
`SpatialDQN`s and the `ReplayBuffer`.  Greedy acting (epsilon = 0), dead agents keep index 0, no training step, batch 1, numpy seed.

Stored -- data only -- per case: the network parameters and their `config`, the ring's tensors, and PER TICK (chronological, also the ticks
a wrapped ring has lost): the actions taken (`taken`), whether the tick ended the episode (`ended`: done or truncated), every agent's Q row
of BOTH networks (`q_imposter [ticks, A, n]`, `q_crew`), the acting episode's imposter mask and the alive flags the loop read
(`imposter_mask`, `alive`), and the flattened state after the tick -- after the reset where the episode ended (`fresh`; `first_state`: the
state the run starts from).  `smallest_argmax_margin` (over the rows actions were taken from: living agents, their own team's network) and
`largest_abs_q` are in the meta.

Condition, asserted here: the smallest argmax margin exceeds 100 x (2e-5 x the largest |Q|), 100 times the tolerance the spatial forward
kernels are held to against torch, so a float32 summation-order difference cannot flip an action.  Seeds are chosen for which it holds.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refshim  # noqa: E402

_refshim.install()
import torch  # noqa: E402

from generate_golden import GRID14, make_env  # noqa: E402
from generate_spatial import every_parameter_matters  # noqa: E402
from src.environment import StateFields  # noqa: E402
from src.features.model_ready import GlobalFeaturizer, PerspectiveFeaturizer  # noqa: E402
from src.models.dqn import SpatialDQN  # noqa: E402
from src.replay_memory import ReplayBuffer  # noqa: E402

OUT_DIR = os.path.join(HERE, "spatial_collect")
MARGIN_FACTOR, KERNEL_TOLERANCE = 100.0, 2e-5  # the condition: margin > MARGIN_FACTOR * KERNEL_TOLERANCE * largest |Q|
SIZE_CAP = 1 << 20


def collect(name, spec, featurizer_cls, net, trajectory_size, max_size, num_steps, seed):
    env = make_env(spec)
    feat = featurizer_cls(env)
    T = trajectory_size
    flat = lambda s: np.asarray(env.flatten_state(s), dtype=np.float64)
    # the featurizer's own shapes, from one fitted window
    np.random.seed(seed)
    state, _ = env.reset()
    feat.fit(torch.tensor(np.stack([flat(state)] * T)).unsqueeze(0))
    sp0, ns0 = feat.generate_featurized_states()[0]
    cfg = dict(net, input_image_size=int(sp0.shape[-1]), non_spatial_input_size=int(ns0.shape[-1]),
               n_channels=[int(sp0.shape[2])] + list(net["n_channels"]))
    models = {}
    for team, n_actions, mseed in (("imposter", env.n_imposter_actions, seed + 100), ("crew", env.n_crew_actions, seed + 200)):
        torch.manual_seed(mseed)
        models[team] = SpatialDQN(**dict(cfg, n_actions=int(n_actions)))
        every_parameter_matters(models[team], mseed)
        models[team].eval()
    buf = ReplayBuffer(max_size, env.flattened_state_size, T, env.n_agents, env.n_imposters)
    np.random.seed(seed)
    # ---- train.py:316-322
    state, _ = env.reset()
    first_state = flat(state)
    state_sequence = np.zeros((buf.trajectory_size, buf.state_size))
    for i in range(buf.trajectory_size):
        state_sequence[i] = env.flatten_state(state)
    taken, ended, fresh, masks, alive_rows, q_rows = [], [], [], [], [], {"imposter": [], "crew": []}
    margins, largest_q = [], 0.0
    for _ in range(num_steps):
        # ---- train.py:345-381 with eps = 0
        feat.fit(torch.tensor(state_sequence).unsqueeze(0))
        agent_actions = np.zeros(env.n_agents, dtype=np.int32)
        alive_agents = np.asarray(state[env.state_fields[StateFields.ALIVE_AGENTS]]).astype(bool)
        imposter_mask = np.asarray(env.imposter_mask).astype(bool)
        tick_q = {"imposter": [], "crew": []}
        with torch.no_grad():
            for agent_idx, (spatial, non_spatial) in enumerate(feat.generate_featurized_states()):
                spatial, non_spatial = spatial.float(), non_spatial.float()
                q = {team: models[team](spatial, non_spatial).reshape(-1) for team in ("imposter", "crew")}
                for team in q:
                    tick_q[team].append(q[team].numpy().copy())
                if not alive_agents[agent_idx]:
                    continue
                own = q["imposter" if imposter_mask[agent_idx] else "crew"]
                agent_actions[agent_idx] = int(torch.argmax(own))
                top = torch.topk(own, 2).values
                margins.append(float(top[0] - top[1]))
                largest_q = max(largest_q, float(own.abs().max()))
        # ---- train.py:383-399
        next_state, reward, done, trunc, info = env.step(agent_actions=agent_actions)
        next_state_sequence = np.roll(state_sequence.copy(), -1, axis=0)
        next_state_sequence[-1] = env.flatten_state(next_state)
        buf.add(state=state_sequence, action=agent_actions, reward=reward, done=done, next_state=next_state_sequence, imposters=env.imposter_idxs)
        taken.append(agent_actions.copy())
        ended.append(int(bool(done or trunc)))
        masks.append(imposter_mask.copy())
        alive_rows.append(alive_agents.copy())
        for team in tick_q:
            q_rows[team].append(np.stack(tick_q[team]))
        # ---- train.py:419-449
        if done or trunc:
            state, _ = env.reset()
            state_sequence = np.zeros((buf.trajectory_size, buf.state_size))
            for i in range(buf.trajectory_size):
                state_sequence[i] = env.flatten_state(state)
        else:
            state = next_state
            state_sequence = next_state_sequence
        fresh.append(flat(state))
    n = buf.size
    bound = MARGIN_FACTOR * KERNEL_TOLERANCE * largest_q
    assert min(margins) > bound, (f"{name}: smallest argmax margin {min(margins)} <= {MARGIN_FACTOR} x {KERNEL_TOLERANCE} x largest |Q| "
                                  f"{largest_q} = {bound}: choose another seed")
    meta = dict(spec)
    meta.update(seed=seed, featurizer=featurizer_cls.__name__, trajectory_size=T, max_size=max_size, num_steps=num_steps,
                state_size=int(env.flattened_state_size), n_agents=int(env.n_agents), n_imposters=int(env.n_imposters), idx=int(buf.idx), size=int(n),
                config=cfg, n_actions={"imposter": int(env.n_imposter_actions), "crew": int(env.n_crew_actions)},
                episodes_ended=int(buf.dones[:n].sum()), windows_refilled=int(np.sum(ended)), dead_agent_ticks=int((~np.array(alive_rows)).sum()),
                smallest_argmax_margin=min(margins), largest_abs_q=largest_q, grid_used=np.asarray(env.grid).astype(int).tolist())
    arrays = {f"{team}::{k}": v.numpy() for team, m in models.items() for k, v in m.state_dict().items()}
    os.makedirs(OUT_DIR, exist_ok=True)
    out = os.path.join(OUT_DIR, f"{name}.npz")
    np.savez_compressed(out, meta=json.dumps(meta), taken=np.array(taken, dtype=np.int16), ended=np.array(ended, dtype=np.uint8),
                        fresh=np.array(fresh).astype(np.int16), first_state=first_state.astype(np.int16),
                        imposter_mask=np.array(masks, dtype=np.uint8), alive=np.array(alive_rows, dtype=np.uint8),
                        q_imposter=np.stack(q_rows["imposter"]).astype(np.float32), q_crew=np.stack(q_rows["crew"]).astype(np.float32),
                        states=buf.states[:n].numpy().astype(np.int16), next_states=buf.next_states[:n].numpy().astype(np.int16),
                        actions=buf.actions[:n].numpy().astype(np.int16), rewards=buf.rewards[:n].numpy().astype(np.float32),
                        dones=buf.dones[:n].numpy().astype(np.uint8), imposters=buf.imposters[:n].numpy().astype(np.int16), **arrays)
    assert os.path.getsize(out) < SIZE_CAP, f"{name}: {os.path.getsize(out)} bytes"
    print(name, "size", n, "idx", buf.idx, "done rows", int(buf.dones[:n].sum()), "windows refilled", int(np.sum(ended)), "dead agent ticks",
          meta["dead_agent_ticks"], "smallest argmax margin", min(margins), "largest |Q|", largest_q, "bound", bound, os.path.getsize(out), "bytes")


def main():
    # (a) the base game 1v3, 5 jobs, on the reference's own 9 x 9 map, episodes of 12 ticks (windows are refilled often), Global featurizer,
    # T = 2 -- the reference's default sequence_length --, a ring that wraps once
    base = dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=3, n_jobs=5, shuffle_imposter_index=False, max_time_steps=12))
    collect("base_1v3_j5_global_t2_wrap", base, GlobalFeaturizer,
            dict(n_channels=[6], strides=[1], paddings=[1], kernel_size=[3, 3], dilations=[1], rnn_layers=1, rnn_hidden_dim=24, rnn_dropout=0.0,
                 mlp_hidden_layer_dims=[16]), 2, 160, 250, 55)  # (a seed whose run has kills: dead agents act)
    # (b) base 1v2, 4 jobs, 14 x 14, Perspective featurizer, T = 3
    base14 = dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=2, n_jobs=4, shuffle_imposter_index=False, max_time_steps=40),
                  grid=GRID14.astype(int).tolist())
    collect("base14_1v2_j4_persp_t3", base14, PerspectiveFeaturizer,
            dict(n_channels=[4], strides=[1], paddings=[1], kernel_size=[3, 3], dilations=[1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0,
                 mlp_hidden_layer_dims=[12]), 3, 256, 150, 48)


if __name__ == "__main__":
    main()
