#!/usr/bin/env python3
"""Golden vectors of the reference trainer's EPISODE BOOKKEEPING (container only).

    python tests/golden/generate_episodes.py        # rewrites tests/golden/episodes/episodes_*.npz

(A directory of their own: every ``*.npz`` directly under tests/golden/ that does not carry one of the known prefixes is replayed as an env
trace by tests/test_oracle_golden.py and tests/test_gpu_parity.py.)

Runs the UNMODIFIED `train()` of src/train.py (284-471) -- with the import stand-ins of generate_train.py -- on the reference env with a
placeholder trainer (`DQNTeamTrainer(None, None, gamma)`: nothing trains, nothing is saved), reference `RandomEquiprobable` models and a
schedule that stays at epsilon = 1, so every action is a numpy draw.  `env.step` is wrapped to record, per tick, what it returned (reward,
done, truncated) and the imposter indices of the episode that acted.  Stored (data only): those per-tick arrays, gamma, and what `train()`
left in its `EpisodicMetricHandler`: the `avg_imposter_returns` / `avg_crew_returns` lists (`G[imposter_mask].mean()`,
`G[~imposter_mask].mean()` at every episode end, train.py:421-422) and the `total_time_steps` history.  `EpisodeLog`'s numpy path
(tests/test_train_loop_host.py) and `susnet_episode_stats` (tests/test_gpu_episodes.py) must reproduce the two return lists bit for bit
from the per-tick arrays.

Conditions asserted here, so that a test cannot pass vacuously: every reward constant is a dyadic rational (the float32 feed carries the
rewards exactly); every file holds at least 20 finished episodes and ends mid-episode; across the set at least 5 episodes of one file end
by truncation, some end by `done`, at least two gammas below 1 are used, and one configuration has a crew of 8 or more (numpy's pairwise
branch of the mean).
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

from generate_golden import GRID14, make_env  # noqa: E402
from src.features import component as comp  # noqa: E402
from src.features.model_ready import FlatFeaturizer  # noqa: E402
from src.metrics import EpisodicMetricHandler, SusMetrics  # noqa: E402
from src.models.dqn import RandomEquiprobable  # noqa: E402
from src.replay_memory import ReplayBuffer  # noqa: E402
from src.scheduler import ExponentialSchedule  # noqa: E402
from src.train import DQNTeamTrainer, train  # noqa: E402

REWARDS = dict(kill_reward=-3, complete_job_reward=1, sabotage_reward=2, time_step_reward=-0.25, game_end_reward=4, dead_penalty=-0.5)
ITG_REWARDS = dict(kill_reward=-3, sabotage_reward=0, end_of_game_reward=2, time_step_reward=-0.25)


def is_dyadic(v) -> bool:
    return float(v) * 1024 == int(float(v) * 1024)


def run(name, spec, gamma, seed, num_steps):
    assert all(is_dyadic(v) for k, v in spec["kwargs"].items() if k.endswith(("reward", "penalty"))), spec
    env = make_env(spec)
    ticks = {"reward": [], "done": [], "trunc": [], "imposters": []}
    inner = env.step

    def step(*a, **k):
        acting = np.array(env.imposter_idxs, dtype=np.int16).copy()  # (the roles of the episode that acts: a reset draws new ones)
        out = inner(*a, **k)
        ticks["reward"].append(np.asarray(out[1], dtype=np.float64).copy())
        ticks["done"].append(bool(out[2]))
        ticks["trunc"].append(bool(out[3]))
        ticks["imposters"].append(acting)
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
        assert not os.listdir(tmp), "a placeholder trainer with random models saves nothing"
    reward = np.array(ticks["reward"])
    assert np.array_equal(reward.astype(np.float32).astype(np.float64), reward), "rewards must be exact in float32"
    done, trunc = np.array(ticks["done"]), np.array(ticks["trunc"])
    ended = done | trunc
    imp_ret = np.array(metrics.metrics[SusMetrics.AVG_IMPOSTER_RETURNS], dtype=np.float64)
    crew_ret = np.array(metrics.metrics[SusMetrics.AVG_CREW_RETURNS], dtype=np.float64)
    steps_hist = np.array(metrics.metrics[SusMetrics.TOTAL_TIME_STEPS], dtype=np.int64)
    n_ep = int(ended.sum())
    assert len(reward) == num_steps and n_ep == len(imp_ret) == len(crew_ret) == len(steps_hist)
    assert n_ep >= 20, (name, n_ep)
    assert not ended[-1], (name, "the run must end mid-episode")
    # length = t_episode + 1 (train.py:430) against the env's own step counter of the episode
    ends = np.flatnonzero(ended)
    length = np.diff(np.concatenate(([-1], ends)))
    assert np.array_equal(length, steps_hist), (name, "t_episode + 1 differs from total_time_steps")
    meta = dict(spec, gamma=gamma, seed=seed, num_steps=num_steps, n_agents=int(env.n_agents), n_imposters=int(env.n_imposters),
                n_crew=int(env.n_crew), episodes=n_ep, ended_by_done=int(done.sum()), ended_by_truncation=int((trunc & ~done).sum()))
    os.makedirs(os.path.join(HERE, "episodes"), exist_ok=True)
    out = os.path.join(HERE, "episodes", f"episodes_{name}.npz")
    np.savez_compressed(out, meta=json.dumps(meta), reward=reward.astype(np.float32), done=done, trunc=trunc,
                        imposters=np.array(ticks["imposters"], dtype=np.int16), gamma=np.float64(gamma), avg_imposter_returns=imp_ret,
                        avg_crew_returns=crew_ret, total_time_steps=steps_hist, length=length.astype(np.int64))
    print(name, "ticks", num_steps, "episodes", n_ep, "done", meta["ended_by_done"], "truncated", meta["ended_by_truncation"],
          os.path.getsize(out), "bytes")
    return meta


def main():
    itg = {"class": "itg", "kwargs": dict(ITG_REWARDS, n_crew=1, n_jobs=0, include_walls=False)}
    base14 = {"class": "base", "kwargs": dict(REWARDS, n_imposters=1, n_crew=2, n_jobs=4, shuffle_imposter_index=True, max_time_steps=25),
              "grid": GRID14.astype(int).tolist()}
    b2v6 = {"class": "base", "kwargs": dict(REWARDS, n_imposters=2, n_crew=6, n_jobs=4, shuffle_imposter_index=True, max_time_steps=120)}
    b1v10 = {"class": "base", "kwargs": dict(REWARDS, n_imposters=1, n_crew=10, n_jobs=3, shuffle_imposter_index=True, max_time_steps=80)}
    b3v9 = {"class": "base", "kwargs": dict(REWARDS, n_imposters=3, n_crew=9, n_jobs=2, shuffle_imposter_index=True, max_time_steps=60)}
    metas = []
    for name, spec, gamma, steps in (("itg_1v1", itg, 0.9, 12000), ("base14_1v2_j4", base14, 0.99, 700), ("base_2v6_j4", b2v6, 0.9, 4000),
                                     ("base_1v10_j3", b1v10, 0.99, 3000), ("base_3v9_j2", b3v9, 0.75, 2500)):
        for seed in (1, 2):
            metas.append(run(f"{name}_s{seed}", spec, gamma, seed, steps + 7 * seed))
    assert len({m["gamma"] for m in metas if m["gamma"] < 1}) >= 2
    assert any(m["ended_by_truncation"] >= 5 for m in metas) and any(m["ended_by_done"] >= 1 for m in metas)
    assert any(m["n_crew"] >= 8 for m in metas)


if __name__ == "__main__":
    main()
