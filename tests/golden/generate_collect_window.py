#!/usr/bin/env python3
"""Golden vectors of the reference trainer's COLLECTION loop on STATE WINDOWS, sequence_length T > 1 (container only).

    python tests/golden/generate_collect_window.py        # rewrites tests/golden/window/wcollect_*.npz

`run_experiment` defaults to `sequence_length=2` (src/train.py:160): the env's last T flattened states form a window, `FlatFeaturizer.fit`
featurizes every state of it (src/features/model_ready.py:325-354) and `MLP.forward` flattens the `[B, T, F]` features into ONE input of
`T * F` values, oldest state first (src/models/dqn.py:86-90).  As in generate_collect.py, `src/train.py` cannot be imported here, so its
acting-and-collecting loop -- train.py:316-322, 345-399 and 419-449 -- is restated around the UNMODIFIED reference objects it drives: the
env, the `FlatFeaturizer`, the Q-networks `MLP([T * F, ...])` and the `ReplayBuffer`.  Greedy acting (epsilon = 0), dead agents keep
index 0, no training step.

Stored -- data only -- is what generate_collect.py stores (the network parameters, the actions taken, the ring's tensors, the smallest
argmax margin), plus: `largest_abs_q`; per ring row whether its transition ENDED the episode (`ended`: done or truncated -- the window
after it is refilled with the fresh first state, train.py:441-445) and the reference featurizer's own `[T * F]` row of the window the
networks acted on (`window_feats`).

Condition, asserted here: the smallest argmax margin of a run exceeds 100 x (2e-5 x the largest |Q|), i.e. 100 times the tolerance the
project's network kernels are held to against torch, so a float32 summation-order difference cannot flip an action.  Seeds are chosen for
which it holds.  The 1v1 case uses generate_collect.py's chase network on the NEWEST segment's columns (zeros elsewhere: the older state
is ignored) with ONE change: the vertical moves' Q values are weighted 9/8.  Unweighted, UP / DOWN and LEFT / RIGHT tie exactly whenever
|dx| = |dy| > 0 (the stored margin of collect_itg_*: 0.0), which no seed avoids; 9 |dy| = 8 |dx| has no solution on a 9 x 9 grid, every
value stays a multiple of 1/8 (exact in float32 in any summation order) and the smallest margin becomes 1/8.
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

from generate_collect import chase_parameters  # noqa: E402
from generate_golden import make_env  # noqa: E402
from src.environment import StateFields  # noqa: E402
from src.features import component as comp  # noqa: E402
from src.features.model_ready import FlatFeaturizer  # noqa: E402
from src.models.dqn import MLP  # noqa: E402
from src.replay_memory import ReplayBuffer  # noqa: E402

OUT_DIR = os.path.join(HERE, "window")
BASE_COMPONENTS = ["onehot_pos", "alive_crew", "closest_crew"]
MARGIN_FACTOR, KERNEL_TOLERANCE = 100.0, 2e-5  # the condition: margin > MARGIN_FACTOR * KERNEL_TOLERANCE * largest |Q|


def chase_on_newest_segment(model, chase, F, T):
    """`chase` = generate_collect.py's `MLP([F, 8, 8, 8, 8, 6])` with `chase_parameters`: its values go into `model` = `MLP([T F, 8, 8, 8, 8,
    6])` with layer 1 on the columns of the window's NEWEST state (the last F) and zeros on the older ones; UP / DOWN weighted 9/8."""
    sd = {k: v.clone() for k, v in chase.state_dict().items()}
    first = next(k for k in sd if k.endswith("weight") and sd[k].dim() == 2)
    last = [k for k in sd if k.endswith("weight") and sd[k].dim() == 2][-1]
    w1 = torch.zeros(sd[first].shape[0], T * F)
    w1[:, (T - 1) * F:] = sd[first]
    sd[first] = w1
    for row in (1, 2):  # UP, DOWN (pred_prey.py:12-19)
        sd[last][row] *= 9.0 / 8.0
        sd[last.replace("weight", "bias")][row] *= 9.0 / 8.0
    model.load_state_dict(sd)


def collect(name, spec, hidden, trajectory_size, max_size, num_steps, seed, components=BASE_COMPONENTS, chase=False):
    env = make_env(spec)
    parts = {"onehot_pos": comp.OneHotAgentPositionFeaturizer, "alive_crew": comp.AliveCrewFeaturizer, "closest_crew": comp.ClosestAliveCrewFeaturizer}
    feat = FlatFeaturizer(env, comp.CompositeFeaturizer([parts[c](env) for c in components]))
    T = trajectory_size
    F = int(feat.featurized_shape[1][0])
    torch.manual_seed(seed)
    imposter_dims = [T * F, *([8, 8, 8, 8] if chase else hidden), int(env.n_imposter_actions)]
    crew_dims = [T * F, *hidden, int(env.n_crew_actions)]
    imposter_model = MLP(list(imposter_dims)).eval()
    crew_model = MLP(list(crew_dims)).eval()
    if chase:
        single = MLP([F, 8, 8, 8, 8, int(env.n_imposter_actions)])
        chase_parameters(single, env.n_cols)
        chase_on_newest_segment(imposter_model, single, F, T)
    buf = ReplayBuffer(max_size, env.flattened_state_size, T, env.n_agents, env.n_imposters)
    ring_ended = np.zeros(max_size, dtype=np.uint8)
    ring_feats = np.zeros((max_size, T * F), dtype=np.uint8)
    np.random.seed(seed)
    # ---- train.py:316-322
    state, _ = env.reset()
    state_sequence = np.zeros((buf.trajectory_size, buf.state_size))
    for i in range(buf.trajectory_size):
        state_sequence[i] = env.flatten_state(state)
    actions, margins, largest_q, episode_ends = [], [], 0.0, 0
    for _ in range(num_steps):
        # ---- train.py:345-381 with eps = 0
        feat.fit(torch.tensor(state_sequence).unsqueeze(0))
        agent_actions = np.zeros(env.n_agents, dtype=np.int32)
        alive_agents = state[env.state_fields[StateFields.ALIVE_AGENTS]]
        window_row = None
        with torch.no_grad():
            for agent_idx, (spatial, non_spatial) in enumerate(feat.generate_featurized_states()):
                if window_row is None:
                    row = non_spatial.detach().reshape(-1).numpy()
                    assert row.shape == (T * F,) and np.array_equal(row, row.astype(np.uint8)), "the flat features are small whole numbers"
                    window_row = row.astype(np.uint8)
                if not alive_agents[agent_idx]:
                    continue
                q = (imposter_model if env.imposter_mask[agent_idx] else crew_model)(spatial, non_spatial).reshape(-1)
                agent_actions[agent_idx] = int(torch.argmax(q))
                top = torch.topk(q, 2).values
                margins.append(float(top[0] - top[1]))
                largest_q = max(largest_q, float(q.abs().max()))
        # ---- train.py:383-399
        next_state, reward, done, trunc, info = env.step(agent_actions=agent_actions)
        next_state_sequence = np.roll(state_sequence.copy(), -1, axis=0)
        next_state_sequence[-1] = env.flatten_state(next_state)
        ring_ended[buf.idx], ring_feats[buf.idx] = int(bool(done or trunc)), window_row  # (the slot `add` writes: replay_memory.py:50-73)
        buf.add(state=state_sequence, action=agent_actions, reward=reward, done=done, next_state=next_state_sequence, imposters=env.imposter_idxs)
        actions.append(agent_actions.copy())
        # ---- train.py:419-449
        if done or trunc:
            episode_ends += 1
            state, _ = env.reset()
            state_sequence = np.zeros((buf.trajectory_size, buf.state_size))
            for i in range(buf.trajectory_size):
                state_sequence[i] = env.flatten_state(state)
        else:
            state = next_state
            state_sequence = next_state_sequence
    n = buf.size
    bound = MARGIN_FACTOR * KERNEL_TOLERANCE * largest_q
    assert min(margins) > bound, (f"{name}: smallest argmax margin {min(margins)} <= {MARGIN_FACTOR} x {KERNEL_TOLERANCE} x largest |Q| "
                                  f"{largest_q} = {bound}: choose another seed")
    meta = dict(spec)
    meta.update(seed=seed, trajectory_size=T, max_size=max_size, num_steps=num_steps, state_size=int(env.flattened_state_size),
                n_agents=int(env.n_agents), n_imposters=int(env.n_imposters), idx=int(buf.idx), size=int(n), components=list(components),
                n_features=F, imposter_dims=imposter_dims, crew_dims=crew_dims, episodes_ended=int(buf.dones[:n].sum()),
                episode_ends_in_run=episode_ends, windows_refilled=int(ring_ended[:n].sum()), smallest_argmax_margin=min(margins),
                largest_abs_q=largest_q, grid_used=np.asarray(env.grid).astype(int).tolist())
    arrays = {"imposter::" + k: v.numpy() for k, v in imposter_model.state_dict().items()}
    arrays.update({"crew::" + k: v.numpy() for k, v in crew_model.state_dict().items()})
    os.makedirs(OUT_DIR, exist_ok=True)
    out = os.path.join(OUT_DIR, f"wcollect_{name}.npz")
    np.savez_compressed(out, meta=json.dumps(meta), taken=np.array(actions, dtype=np.int16), states=buf.states[:n].numpy().astype(np.int16),
                        next_states=buf.next_states[:n].numpy().astype(np.int16), actions=buf.actions[:n].numpy().astype(np.int16),
                        rewards=buf.rewards[:n].numpy().astype(np.float32), dones=buf.dones[:n].numpy().astype(np.uint8),
                        imposters=buf.imposters[:n].numpy().astype(np.int16), ended=ring_ended[:n], window_feats=ring_feats[:n], **arrays)
    print(name, "size", n, "idx", buf.idx, "done rows", int(buf.dones[:n].sum()), "windows refilled", int(ring_ended[:n].sum()),
          "smallest argmax margin", min(margins), "largest |Q|", largest_q, "bound", bound, os.path.getsize(out), "bytes")


def main():
    # the base game of BASELINE config 2's shape on the reference's own 9 x 9 map: episodes of 12 ticks, so windows are refilled often
    base = dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=3, n_jobs=5, shuffle_imposter_index=False, max_time_steps=12))
    collect("base_1v3_j5_t2_wrap", base, [32, 32, 16, 16], 2, 160, 250, 31)  # the ring wraps once
    collect("base_1v3_j5_t3", base, [24, 16, 16], 3, 256, 200, 32)
    # episodes that END BY KILLS: the 1v1 game of notebooks/experiment_1v1.ipynb, the chase network on the newest state's columns
    itg = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
    collect("itg_1v1_nowalls_kills_t2", dict(**{"class": "itg"}, kwargs=dict(itg, include_walls=False)), [32, 32, 16, 16], 2, 256, 220, 33,
            components=["onehot_pos"], chase=True)


if __name__ == "__main__":
    main()
