"""The reference's training loop, ``train()`` / ``run_experiment()`` (src/train.py:152-471), for B environments in lockstep on the device.

The reference does, per tick ``t``: checkpoint if ``t in t_saves``, target sync if ``t % target_update_interval == 0``, act
(epsilon-greedy), step, ``replay_buffer.add``, and a train step if ``t % train_step_interval == 0``; at each episode end it records the
teams' returns.  Here the ticks between two train steps are ONE block: one ``DeviceReplayBuffer.collect`` (one rollout launch + one ring
append), one ``EpisodeLog.update`` on the block's feed, and at most one ``DeviceDQNTeamTrainer.train_step``.  The weights only change in a
train step and the target networks are only read by one, so a checkpoint or a target sync due at any tick of a block is done before the
block: the same weights are saved, the same weights are copied.  ``plan_blocks`` is that schedule as data.

One deviation: epsilon is one value per block, ``scheduler.value(first tick of the block)``, because a rollout launch takes one epsilon
(the reference evaluates the schedule every tick, train.py:351).  With ``train_step_interval=1`` every block is one tick and it vanishes.

Nothing is read back inside the loop: losses go to a preallocated device tensor, episodes to the ``EpisodeLog``; both are copied to the
host once, after the last block.  (Writing a checkpoint copies weights to the host: at most ``num_saves - 1`` times per run.)
"""
from __future__ import annotations

import json
import pathlib
from collections import namedtuple
from datetime import datetime
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .episodes import EpisodeLog
from .metrics import EpisodicMetricHandler, SusMetrics
from .policy import MLP, PolicyRollout, RandomEquiprobable, SpatialDQN
from .replay import DeviceReplayBuffer
from .scheduler import ExponentialSchedule
from .trainer import DeviceDQNTeamTrainer

Block = namedtuple("Block", ("t0", "n_ticks", "sync_ticks", "save_ticks", "trains"))
Block.__doc__ = """Ticks ``t0 .. t0 + n_ticks - 1``; ``sync_ticks`` / ``save_ticks``: the ticks inside the block at which the reference syncs the
targets / writes a checkpoint (both done before the block); ``trains``: the block's last tick is a train tick."""


def save_ticks(num_steps: int, num_saves: int) -> np.ndarray:
    """train.py:310."""
    return np.linspace(0, num_steps, num_saves - 1, endpoint=False, dtype=int)


def plan_blocks(num_steps: int, train_step_interval: int = 5, target_update_interval: int = 10_000, num_saves: int = 5) -> List[Block]:
    """The block schedule of ``train()``: a first block of one tick (tick 0 trains), then blocks that end on the next multiple of
    ``train_step_interval``, and a shorter last block that ends with the run."""
    num_steps, k, u = int(num_steps), int(train_step_interval), int(target_update_interval)
    assert k >= 1 and u >= 1, "train_step_interval and target_update_interval must be positive"
    saves = sorted(set(int(t) for t in save_ticks(num_steps, num_saves))) if num_steps > 0 else []
    blocks, t0 = [], 0
    while t0 < num_steps:
        end = min(-(-t0 // k) * k, num_steps - 1)  # the next train tick at or after t0, or the run's last tick
        n = end - t0 + 1
        first_sync = -(-t0 // u) * u
        blocks.append(Block(t0, n, tuple(range(first_sync, end + 1, u)), tuple(t for t in saves if t0 <= t <= end), end % k == 0))
        t0 = end + 1
    return blocks


def model_type(model) -> str:
    """The reference's ``ModelType`` value of a model (dqn.py:9-12), as its checkpoint names spell it."""
    if model is None or isinstance(model, RandomEquiprobable):
        return "random"
    if isinstance(model, MLP):
        return "mlp"
    if isinstance(model, SpatialDQN):
        return "spatial_dqn"
    raise TypeError(f"no reference model type for {type(model).__name__}")


def checkpoint_name(team: str, model, progress) -> str:
    """train.py:333-338 (``progress`` = ``int(t * 100 / num_steps)``) and 453-457 (``progress`` = ``"100%"``)."""
    return f"{team}_{model_type(model)}_{progress}.pt"


def _save(models, directory: pathlib.Path, progress) -> None:
    for team, model in zip(("imposter", "crew"), models):
        if model is not None and hasattr(model, "dump_to_checkpoint") and not isinstance(model, RandomEquiprobable):  # (dqn.py:131-132: a random model saves nothing)
            model.dump_to_checkpoint(directory / checkpoint_name(team, model, progress))


# the info counters the reference's handler keeps per episode (metrics.py:22-32 + the two outcome flags) <- the env's lifetime accumulators
_LIFETIME_OF = {SusMetrics.IMP_KILLED_CREW: "imp_killed_crew", SusMetrics.IMP_VOTED_OUT: "imp_voted_out", SusMetrics.CREW_VOTED_OUT: "crew_voted_out",
                SusMetrics.SABOTAGED_JOBS: "sabotaged_jobs", SusMetrics.COMPLETED_JOBS: "completed_jobs", SusMetrics.TOTAL_STALEMATES: None,
                SusMetrics.TOTAL_TIME_STEPS: "episode_steps", SusMetrics.IMPOSTER_WON: "imposter_won", SusMetrics.CREW_WON: "crew_won"}


def train(env, metrics: EpisodicMetricHandler, num_steps: int, replay_buffer: DeviceReplayBuffer, policy: PolicyRollout,
          trainer: DeviceDQNTeamTrainer, scheduler: ExponentialSchedule, save_directory_path, train_step_interval: int = 5,
          batch_size: int = 32, num_saves: int = 5, target_update_interval: int = 10_000, generator: Optional[torch.Generator] = None,
          episode_log: Optional[EpisodeLog] = None) -> EpisodeLog:
    """``train()`` of src/train.py:284-471.  ``num_steps`` counts lockstep ticks: each adds ``env.batch`` transitions.  ``policy``: the
    ``PolicyRollout`` the teams act by (reference MLPs the Q-network kernel serves; a crew model of None = random crew); ``trainer``: the
    ``DeviceDQNTeamTrainer`` over the same models (built with ``policy=policy``, so that acting follows the trained weights);
    ``generator``: draws the replay samples.  ``metrics`` receives what the reference's handler holds after its ``train()``; the
    ``EpisodeLog`` (returned) keeps tick, env, length and cause of every episode as well."""
    if not env.auto_reset:
        raise ValueError("train: the env must be built with auto_reset=True (episodes restart inside the rollout launch)")
    if policy.env is not env or trainer.env is not env:
        raise ValueError("train: policy and trainer must be built over the env that is trained on")
    if policy.fused_imposter is None or (policy.crew_model is not None and policy.fused_crew is None):
        raise ValueError("train: served are reference MLPs on a compiled-in feature layout (PolicyRollout.fused_imposter / fused_crew); "
                         "a crew model of None acts randomly")
    save_dir = pathlib.Path(save_directory_path)
    trains = any(trainer.trained)
    blocks = plan_blocks(num_steps, train_step_interval, target_update_interval, num_saves)
    losses = torch.zeros(sum(b.trains for b in blocks), 2, dtype=torch.float32, device=env.device)
    save_dir.mkdir(parents=True, exist_ok=True)

    env.reset()  # train.py:316
    first_record = 0
    if episode_log is None:
        episode_log = EpisodeLog(env, gamma=trainer.gamma)
    else:  # a log that is carried through several runs: this run's episodes start behind what it holds
        first_record = episode_log.records()["count"]
        episode_log.reset(keep_log=True)
    life0 = env.lifetime_totals().clone()
    k_train = 0
    for blk in blocks:
        if trains:
            for t in blk.save_ticks:  # train.py:331-338
                _save(trainer.models, save_dir, int(t * 100 / num_steps))
        if blk.sync_ticks:  # train.py:341-343
            trainer.sync_targets()
        replay_buffer.collect(env, policy, blk.n_ticks, epsilon=float(scheduler.value(blk.t0)), ticks_per_append=blk.n_ticks)
        feed, n = replay_buffer.last_feed
        episode_log.update(feed, n, tick_base=blk.t0)  # (`tick` counts from this run's first tick, also in a log carried over)
        if blk.trains:  # train.py:402-416
            if trains:
                losses[k_train].copy_(trainer.train_step(replay_buffer, batch_size, generator))
            k_train += 1
    _save(trainer.models, save_dir, "100%")  # train.py:453-457 (written whether or not anything trained, as there)

    # ---- the only read-back: the episode log, the loss history, the lifetime totals ----
    rec = episode_log.records()
    life = (env.lifetime_totals() - life0).cpu().tolist()
    loss_rows = losses.cpu().tolist()
    metrics.set({SusMetrics.AVG_IMPOSTER_RETURNS: rec["imposter_return"][first_record:].tolist(),
                 SusMetrics.AVG_CREW_RETURNS: rec["crew_return"][first_record:].tolist()})
    metrics.set({SusMetrics.IMPOSTER_LOSS: [r[0] for r in loss_rows], SusMetrics.CREW_LOSS: [r[1] for r in loss_rows]})
    # one entry per counter: its mean per finished episode over the run (per-episode histories would need the stepping kernels to emit them)
    episodes = life[L.LIFETIME_NAMES.index("episodes")]
    metrics.set({m: [(life[L.LIFETIME_NAMES.index(name)] / max(episodes, 1)) if name else 0.0] for m, name in _LIFETIME_OF.items()})
    return episode_log


def run_experiment(env, num_steps: int, imposter_model, crew_model, components: Sequence[str], sequence_length: int = 1,
                   replay_buffer_size: int = 100_000, replay_prepopulate_steps: int = 1000, batch_size: int = 32, gamma: float = 0.99,
                   scheduler_start_eps: float = 1.0, scheduler_end_eps: float = 0.05, scheduler_time_steps: int = 1_000_000,
                   train_imposter: bool = True, train_crew: bool = True, experiment_base_dir=None, learning_rate: float = 0.0001,
                   train_step_interval: int = 5, num_checkpoint_saves: int = 5, target_update_interval: int = 10_000,
                   generator: Optional[torch.Generator] = None, episode_log: Optional[EpisodeLog] = None) -> EpisodicMetricHandler:
    """``run_experiment`` of src/train.py:152-281 with the models given as modules: writes ``config.json``, builds ring, policy, trainer
    and schedule, pre-populates the ring with ``replay_prepopulate_steps`` random ticks, runs ``train()``, writes ``metrics.json`` and the
    checkpoints into ``experiment_base_dir/<timestamp>/`` and returns the metric handler.  ``replay_buffer_size`` counts transitions."""
    components = list(components)
    if env.obs_config.mode != "flat" or list(env.obs_config.components) != components:
        raise ValueError("run_experiment: build the env with obs=ObsConfig('flat', components), auto_reset=True")
    if sequence_length != 1:
        raise ValueError("run_experiment: a window of one state is served (sequence_length=1): the Q-network kernel and "
                         "susnet_dqn_train_step read one state")
    if not isinstance(imposter_model, MLP) or not (crew_model is None or isinstance(crew_model, MLP)):
        raise ValueError("run_experiment: served are reference MLPs (a crew model of None acts randomly)")
    base = pathlib.Path(experiment_base_dir) if experiment_base_dir is not None else pathlib.Path.cwd() / "model_registry" / "experiments"
    experiment_dir = base / datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
    experiment_dir.mkdir(parents=True, exist_ok=True)
    config = {
        "num_steps": num_steps, "batch": env.batch, "imposter_model_args": getattr(imposter_model, "config", None),
        "crew_model_args": getattr(crew_model, "config", None), "imposter_model_type": model_type(imposter_model),
        "crew_model_type": model_type(crew_model), "featurizer_type": "flat:" + "+".join(components), "sequence_length": sequence_length,
        "replay_buffer_size": replay_buffer_size, "replay_prepopulate_steps": replay_prepopulate_steps, "batch_size": batch_size, "gamma": gamma,
        "scheduler_start_eps": scheduler_start_eps, "scheduler_end_eps": scheduler_end_eps, "scheduler_time_steps": scheduler_time_steps,
        "train_imposter": train_imposter, "train_crew": train_crew, "experiment_base_dir": str(base), "optimizer_type": "adam",
        "learning_rate": learning_rate, "train_step_interval": train_step_interval, "target_update_interval": target_update_interval,
    }
    (experiment_dir / "config.json").write_text(json.dumps(config, indent=4, default=str))

    policy = PolicyRollout(env, imposter_model, crew_model, components=components, mask_dead=True)
    trainer = DeviceDQNTeamTrainer(env, imposter_model, crew_model, components, lr=learning_rate, gamma=gamma, train_imposter=train_imposter,
                                   train_crew=train_crew, policy=policy)
    scheduler = ExponentialSchedule(scheduler_start_eps, scheduler_end_eps, scheduler_time_steps)
    metrics = EpisodicMetricHandler()
    ring = DeviceReplayBuffer(replay_buffer_size, env.flattened_state_size, sequence_length, env.n_agents, env.n_imposters, device=env.device)
    if replay_prepopulate_steps > 0:
        ring.populate_fused(env, replay_prepopulate_steps)
    train(env, metrics, num_steps, ring, policy, trainer, scheduler, experiment_dir, train_step_interval=train_step_interval,
          batch_size=batch_size, num_saves=num_checkpoint_saves, target_update_interval=target_update_interval, generator=generator,
          episode_log=episode_log)
    metrics.save_metrics(save_file_path=experiment_dir / "metrics.json")
    return metrics
