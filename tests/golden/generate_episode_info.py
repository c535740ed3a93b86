#!/usr/bin/env python3
"""Golden vectors of the reference trainer's PER-EPISODE INFO COUNTERS (container only).

    python tests/golden/generate_episode_info.py        # rewrites tests/golden/episodes/epinfo_*.npz

Runs the UNMODIFIED `train()` of src/train.py (284-471) as generate_episodes.py does (placeholder trainer, reference `RandomEquiprobable`
models, epsilon = 1: every action is a numpy draw) and records, per tick, what `env.step` returned -- reward, done, truncated, the imposter
indices of the episode that acted and the nine counters of the `info` dict (SusMetrics order: imp_killed_crew, imp_voted_out,
crew_voted_out, sabotaged_jobs, completed_jobs, total_stalemates, total_time_steps, imposter_won, crew_won).  Stored next to them (data
only): what `metrics.step(info)` appended at every episode end (train.py:419-427) -- the nine per-episode lists of the run's
`EpisodicMetricHandler` -- and the two return lists.  `EpisodeLog`'s numpy path with an `ep_info` array must reproduce the per-episode
lists from the per-tick rows exactly (tests/test_episode_info_host.py).

(The prefix is `epinfo_`, not `episodes_`: the fixtures of generate_episodes.py are enumerated by that prefix.)

Conditions asserted here, so that a test cannot pass vacuously: each file holds at least 20 finished episodes and ends mid-episode; across
the set crew members are killed, jobs are completed, imposters win, and episodes have more than one length.  (The reference's random
trainer policy rarely votes or sabotages: those counters are pinned on the GPU against the step traces under tests/golden/.)
"""
from __future__ import annotations

import json
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_train  # noqa: E402,F401  (installs the reference import shims and the stand-ins src/train.py needs)
import torch  # noqa: E402

from generate_episodes import REWARDS  # noqa: E402
from generate_golden import GRID14, make_env  # noqa: E402
from src.features import component as comp  # noqa: E402
from src.features.model_ready import FlatFeaturizer  # noqa: E402
from src.metrics import EpisodicMetricHandler, SusMetrics  # noqa: E402
from src.models.dqn import RandomEquiprobable  # noqa: E402
from src.replay_memory import ReplayBuffer  # noqa: E402
from src.scheduler import ExponentialSchedule  # noqa: E402
from src.train import DQNTeamTrainer, train  # noqa: E402

INFO = [SusMetrics.IMP_KILLED_CREW, SusMetrics.IMP_VOTED_OUT, SusMetrics.CREW_VOTED_OUT, SusMetrics.SABOTAGED_JOBS, SusMetrics.COMPLETED_JOBS,
        SusMetrics.TOTAL_STALEMATES, SusMetrics.TOTAL_TIME_STEPS, SusMetrics.IMPOSTER_WON, SusMetrics.CREW_WON]


def run(name, spec, gamma, seed, num_steps):
    env = make_env(spec)
    ticks = {"reward": [], "done": [], "trunc": [], "imposters": [], "info": []}
    inner = env.step

    def step(*a, **k):
        acting = np.array(env.imposter_idxs, dtype=np.int16).copy()  # (the roles of the episode that acts: a reset draws new ones)
        out = inner(*a, **k)
        ticks["reward"].append(np.asarray(out[1], dtype=np.float64).copy())
        ticks["done"].append(bool(out[2]))
        ticks["trunc"].append(bool(out[3]))
        ticks["imposters"].append(acting)
        ticks["info"].append([int(out[4][m]) for m in INFO])
        return out

    env.step = step
    feat = FlatFeaturizer(env, comp.CompositeFeaturizer([comp.OneHotAgentPositionFeaturizer(env)]))
    imposter_model, crew_model = RandomEquiprobable(env.n_imposter_actions), RandomEquiprobable(env.n_crew_actions)
    metrics = EpisodicMetricHandler()
    buf = ReplayBuffer(max_size=64, trajectory_size=1, state_size=env.flattened_state_size, n_imposters=env.n_imposters, n_agents=env.n_agents)
    np.random.seed(seed)
    torch.manual_seed(seed)
    with tempfile.TemporaryDirectory() as tmp:
        train(env=env, metrics=metrics, num_steps=num_steps, replay_buffer=buf, featurizer=feat, imposter_model=imposter_model,
              crew_model=crew_model, scheduler=ExponentialSchedule(1.0, 1.0, 10), save_directory_path=pathlib.Path(tmp),
              trainer=DQNTeamTrainer(None, None, gamma), gamma=gamma)
    reward = np.array(ticks["reward"])
    assert np.array_equal(reward.astype(np.float32).astype(np.float64), reward), "rewards must be exact in float32"
    done, trunc, info = np.array(ticks["done"]), np.array(ticks["trunc"]), np.array(ticks["info"], dtype=np.int64)
    ended = done | trunc
    n_ep = int(ended.sum())
    per_episode = np.array([[int(v) for v in metrics.metrics[m]] for m in INFO], dtype=np.int64).T  # [episodes][9]
    assert per_episode.shape == (n_ep, len(INFO)), (name, per_episode.shape, n_ep)
    assert n_ep >= 20 and not ended[-1], (name, n_ep)
    meta = dict(spec, gamma=gamma, seed=seed, num_steps=num_steps, n_agents=int(env.n_agents), n_imposters=int(env.n_imposters),
                n_crew=int(env.n_crew), episodes=n_ep, info_names=[m.value for m in INFO])
    os.makedirs(os.path.join(HERE, "episodes"), exist_ok=True)
    out = os.path.join(HERE, "episodes", f"epinfo_{name}.npz")
    np.savez_compressed(out, meta=json.dumps(meta), reward=reward.astype(np.float32), done=done, trunc=trunc,
                        imposters=np.array(ticks["imposters"], dtype=np.int16), gamma=np.float64(gamma), info=info.astype(np.int32),
                        episode_info=per_episode.astype(np.int32),
                        avg_imposter_returns=np.array(metrics.metrics[SusMetrics.AVG_IMPOSTER_RETURNS], dtype=np.float64),
                        avg_crew_returns=np.array(metrics.metrics[SusMetrics.AVG_CREW_RETURNS], dtype=np.float64))
    print(name, "ticks", num_steps, "episodes", n_ep, "column sums", per_episode.sum(axis=0).tolist(), os.path.getsize(out), "bytes")
    return per_episode


def main():
    tagging = {"class": "tagging", "kwargs": dict(REWARDS, vote_reward=2, n_imposters=1, n_crew=4, n_jobs=5, shuffle_imposter_index=True,
                                                  max_time_steps=60, tag_reset_interval=3)}
    base = {"class": "base", "kwargs": dict(REWARDS, n_imposters=1, n_crew=2, n_jobs=4, shuffle_imposter_index=True, max_time_steps=80)}
    tag = np.concatenate([run(f"tagging_1v4_j5_int3_s{seed}", tagging, 0.9, seed, 4000 + 7 * seed) for seed in (1, 2)])
    jobs = np.concatenate([run(f"base_1v2_j4_s{seed}", base, 0.99, seed, 5000 + 7 * seed) for seed in (1, 2)])
    col = {m.value: i for i, m in enumerate(INFO)}
    both = np.concatenate([tag, jobs])
    for k in ("imp_killed_crew", "completed_jobs", "total_time_steps", "imposter_won"):
        assert both[:, col[k]].sum() > 0, k
    assert len(set(both[:, col["total_time_steps"]].tolist())) > 1, "episodes of more than one length"

if __name__ == "__main__":
    main()
