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

import dataclasses
import json
import os
import pathlib
from collections import namedtuple
from datetime import datetime
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .episodes import EpisodeLog
from .metrics import EpisodicMetricHandler, SusMetrics
from .policy import (MLP, BlockActor, PolicyRollout, RandomEquiprobable, SpatialDQN, WindowedPolicyRollout, acting_kind, check_policy_step_actions,
                     check_random_crew_stream, spatial_desc, spatial_feed_mismatch)
from .replay import DeviceReplayBuffer
from .scheduler import ExponentialSchedule
from .trainer import DeviceDQNSweepTrainer, DeviceDQNTeamTrainer

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


def stop_boundary(blocks: List[Block], stop_after: int) -> Optional[int]:
    """Where ``stop_after=t`` stops a run of ``blocks``: the completed ticks at the first block boundary with at least ``t`` of them (a
    boundary lies behind a block's train step, or behind its collect when the block does not train: 1, k+1, 2k+1, ... and the run's
    end), or None when ``t`` lies beyond the run -- it then finishes."""
    t = int(stop_after)
    for blk in blocks:
        if blk.t0 + blk.n_ticks >= t:
            return blk.t0 + blk.n_ticks
    return None


def snapshot_boundaries(blocks: List[Block], snapshot_interval: int) -> List[int]:
    """Where ``snapshot_interval=n`` writes ``run_state.pt``: the completed ticks at the first block boundary at or beyond every ``n``
    completed ticks.  The run's end is no such boundary: the run finishes there instead."""
    n = int(snapshot_interval)
    if n < 1:
        raise ValueError(f"snapshot_interval = {snapshot_interval}: a positive number of ticks")
    out, due = [], n
    for blk in blocks[:-1]:
        done = blk.t0 + blk.n_ticks
        if done >= due:
            out.append(done)
            due = n * (done // n + 1)
    return out


RUN_STATE_FILE = "run_state.pt"
RUN_STATE_FORMAT = 1


def write_run_state(directory, state: dict) -> pathlib.Path:
    """``state`` as ``directory/run_state.pt``, atomically: written under a temporary name in the same directory, then ``os.replace``d.
    A write that fails leaves no partial file under the final name, and the previous snapshot where it was."""
    directory = pathlib.Path(directory)
    path, tmp = directory / RUN_STATE_FILE, directory / f".{RUN_STATE_FILE}.{os.getpid()}.tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()
    return path


def read_run_state(directory) -> dict:
    """The snapshot ``directory/run_state.pt`` as ``write_run_state`` wrote it (host tensors and plain values).  Refused, each with its
    own message: a directory without the file (``FileNotFoundError``), a file written under another ``SUSNET_ABI_VERSION`` or snapshot
    format, and the snapshot of a finished run (``ValueError``)."""
    path = pathlib.Path(directory) / RUN_STATE_FILE
    if not path.is_file():
        raise FileNotFoundError(f"resume_from={str(directory)!r}: there is no {RUN_STATE_FILE} (a run writes one with snapshot_interval= or "
                                "stop_after=)")
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("format") != RUN_STATE_FORMAT:
        raise ValueError(f"{path}: not a run snapshot of format {RUN_STATE_FORMAT} (format: {state.get('format') if isinstance(state, dict) else None!r})")
    if state.get("abi_version") != L.ABI_VERSION:
        raise ValueError(f"{path}: written under SUSNET_ABI_VERSION {state.get('abi_version')}, this library is version {L.ABI_VERSION}: the "
                         "state blob of one version is not read by another")
    if state.get("finished"):
        raise ValueError(f"{path}: the snapshot of a finished run ({state.get('completed_ticks')} ticks, checkpoints and metrics written): "
                         "there is nothing to resume")
    return state


def check_resume_config(who: str, config: dict, directory) -> None:
    """``ValueError`` unless the ``config.json`` this call would write equals the one in ``directory`` on every key but
    ``experiment_base_dir``; the message names the key and both values.  Reads only."""
    path = pathlib.Path(directory) / "config.json"
    if not path.is_file():
        raise FileNotFoundError(f"{who}: resume_from={str(directory)!r}: there is no config.json: not a run's directory")
    theirs, mine = json.loads(path.read_text()), json.loads(json.dumps(config, default=str))
    absent = "<absent>"
    for key in list(mine) + [k for k in theirs if k not in mine]:
        if key != "experiment_base_dir" and mine.get(key, absent) != theirs.get(key, absent):
            raise ValueError(f"{who}: resume_from={str(directory)!r}: {key} is {mine.get(key, absent)!r} in this call and "
                             f"{theirs.get(key, absent)!r} in the run's config.json: a run is resumed with the arguments it was started with")


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


# the info counters the reference's handler keeps per episode (metrics.py:22-32 + the two outcome flags) <- EpisodeLog.records() arrays
# (None: total_stalemates, which the reference never increments -- a zero per episode)
_RECORD_OF = {SusMetrics.IMP_KILLED_CREW: "imp_killed_crew", SusMetrics.IMP_VOTED_OUT: "imp_voted_out", SusMetrics.CREW_VOTED_OUT: "crew_voted_out",
              SusMetrics.SABOTAGED_JOBS: "sabotaged_jobs", SusMetrics.COMPLETED_JOBS: "completed_jobs", SusMetrics.TOTAL_STALEMATES: None,
              SusMetrics.TOTAL_TIME_STEPS: "total_time_steps", SusMetrics.IMPOSTER_WON: "imposter_won", SusMetrics.CREW_WON: "crew_won"}


# ... and <- the env's lifetime accumulators (the one-mean-per-counter form)
_LIFETIME_OF = {SusMetrics.IMP_KILLED_CREW: "imp_killed_crew", SusMetrics.IMP_VOTED_OUT: "imp_voted_out", SusMetrics.CREW_VOTED_OUT: "crew_voted_out",
                SusMetrics.SABOTAGED_JOBS: "sabotaged_jobs", SusMetrics.COMPLETED_JOBS: "completed_jobs", SusMetrics.TOTAL_STALEMATES: None,
                SusMetrics.TOTAL_TIME_STEPS: "episode_steps", SusMetrics.IMPOSTER_WON: "imposter_won", SusMetrics.CREW_WON: "crew_won"}


def info_metric_lists(rec, first_record: int = 0):
    """``{SusMetrics: [one value per episode]}`` for the nine info counters from ``EpisodeLog.records()`` (a log fed with ``ep_info``), in
    episode order: what the reference's handler holds after ``metrics.step(info)`` at every episode end (train.py:419-427)."""
    n = len(rec["tick"]) - first_record
    return {m: (rec[name][first_record:].tolist() if name else [0] * n) for m, name in _RECORD_OF.items()}


class _Run:
    """One learner's side of the block loop: what ``train()`` does around the train step.  ``train()`` drives one of these,
    ``train_sweep()`` several in lockstep -- the same methods in the same order per member."""

    def __init__(self, who, env, metrics, num_steps, replay_buffer, policy, trainer, scheduler, save_directory_path, blocks, generator=None,
                 episode_log=None, per_episode_info=False, schedule=None, resume=None):
        if not env.auto_reset:
            raise ValueError(f"{who}: the env must be built with auto_reset=True (episodes restart inside the rollout launch)")
        if policy.env is not env or trainer.env is not env:
            raise ValueError(f"{who}: policy and trainer must be built over the env that is trained on")
        kind, imp_served, crew_served = acting_kind(policy)
        if not imp_served or not crew_served:
            raise ValueError(f"{who}: served are reference MLPs a network kernel runs (PolicyRollout.fused_imposter / fused_crew on the compiled-in "
                             "feature layouts, dense_imposter / dense_crew elsewhere: PolicyRollout(..., dense=True)) and SpatialDQNs "
                             "susnet_spatial_forward runs (spatial_imposter / spatial_crew: WindowedPolicyRollout(..., kernels=True)); a crew "
                             "model of None acts randomly")
        if kind == "per_agent":
            check_random_crew_stream(who, env, policy)
        if kind == "dense":  # (a random crew off the philox stream is collect's to refuse)
            check_policy_step_actions(who, env)
        self.env, self.metrics, self.num_steps, self.ring, self.policy, self.trainer = env, metrics, num_steps, replay_buffer, policy, trainer
        self.scheduler, self.generator, self.per_episode_info = scheduler, generator, per_episode_info
        self.save_dir = pathlib.Path(save_directory_path)
        self.trains = any(trainer.trained)
        self.losses = torch.zeros(sum(b.trains for b in blocks), 2, dtype=torch.float32, device=env.device)
        self.who, self.schedule, self.finished = who, dict(schedule or {}, num_steps=int(num_steps), per_episode_info=bool(per_episode_info)), False
        if resume is not None:  # (its checks come before the first write: a refused resume leaves the directory as it was)
            self._check_resume(resume)
        self.save_dir.mkdir(parents=True, exist_ok=True)

        if resume is not None:  # no env.reset(): the env, like everything else, goes on from the snapshot
            self.episode_log = episode_log if episode_log is not None else EpisodeLog(env, gamma=trainer.gamma)
            self._load(resume)
            return
        env.reset()  # train.py:316
        self.first_record = 0
        if episode_log is None:
            episode_log = EpisodeLog(env, gamma=trainer.gamma)
        else:  # a log that is carried through several runs: this run's episodes start behind what it holds
            self.first_record = episode_log.records()["count"]
            episode_log.reset(keep_log=True)
        self.episode_log = episode_log
        self.life0 = None if per_episode_info else env.lifetime_totals().clone()

    # ---- snapshot / resume ----
    def state_dict(self, completed_ticks: int, train_steps: int) -> dict:
        """The run at a block boundary, as host tensors and plain values: every object's ``state_dict`` (env, ring, trainer, policy,
        episode log), the sample generator's state (the caller's generator, or without one the device's global generator), and the
        run's own: completed ticks, the rows of the loss history written so far, ``first_record`` and the lifetime baseline.  The one
        place where the loop waits for the device and copies to the host."""
        env, g = self.env, self.generator
        with torch.cuda.device(env.device):
            return {"format": RUN_STATE_FORMAT, "abi_version": L.ABI_VERSION, "finished": bool(self.finished), "schedule": dict(self.schedule),
                    "completed_ticks": int(completed_ticks), "train_steps": int(train_steps), "losses": self.losses[:train_steps].cpu(),
                    "first_record": int(self.first_record), "life0": None if self.life0 is None else self.life0.cpu(),
                    "env": env.state_dict(), "ring": self.ring.state_dict(), "trainer": self.trainer.state_dict(),
                    "policy": self.policy.state_dict(), "episode_log": self.episode_log.state_dict(),
                    "generator": {"own": g is not None, "state": g.get_state() if g is not None else torch.cuda.get_rng_state(env.device)}}

    def snapshot(self, completed_ticks: int, train_steps: int) -> pathlib.Path:
        return write_run_state(self.save_dir, self.state_dict(completed_ticks, train_steps))

    def _check_resume(self, state: dict) -> None:
        """What can be told without touching an object: the snapshot's schedule is this run's, and it has a sample generator of the kind
        this run draws from."""
        for key, mine in self.schedule.items():
            theirs = state["schedule"].get(key)
            if theirs != mine:
                raise ValueError(f"{self.who}: resume: {key} is {mine!r} in this call and {theirs!r} in the snapshot: a run is resumed with "
                                 "the arguments it was started with")
        if bool(state["generator"]["own"]) != (self.generator is not None):
            raise ValueError(f"{self.who}: resume: the run drew its samples from " + ("a generator of its own" if state["generator"]["own"] else
                             "the device's global generator") + ": pass " + ("one" if state["generator"]["own"] else "none") + " again")
        if int(state["completed_ticks"]) > self.num_steps or int(state["train_steps"]) > self.losses.shape[0]:
            raise ValueError(f"{self.who}: resume: the snapshot holds {state['completed_ticks']} ticks, the run has {self.num_steps}")

    def _load(self, state: dict) -> None:
        """The snapshot into the freshly built objects: env first (the ring keys its carried window to the env's ``reset_generation``),
        then ring, trainer (in place: the policy's models are the trainer's), policy (its forced ``refresh_weights``), episode log,
        generator, and the run's own values."""
        env = self.env
        env.load_state_dict(state["env"])
        self.ring.load_state_dict(state["ring"], env)
        self.trainer.load_state_dict(state["trainer"])
        self.policy.load_state_dict(state["policy"])
        self.episode_log.load_state_dict(state["episode_log"])
        if self.generator is not None:
            self.generator.set_state(state["generator"]["state"])
        else:
            torch.cuda.set_rng_state(state["generator"]["state"], env.device)
        k = int(state["train_steps"])
        self.losses[:k].copy_(state["losses"])
        self.first_record = int(state["first_record"])
        self.life0 = None if state["life0"] is None else state["life0"].to(env.device)

    def before_train_step(self, blk: Block) -> None:
        """The block up to its train step: checkpoints and target sync due inside it, the collect, the episode bookkeeping."""
        if self.trains:
            for t in blk.save_ticks:  # train.py:331-338
                _save(self.trainer.models, self.save_dir, int(t * 100 / self.num_steps))
        if blk.sync_ticks:  # train.py:341-343
            self.trainer.sync_targets()
        self.ring.collect(self.env, self.policy, blk.n_ticks, epsilon=float(self.scheduler.value(blk.t0)), ticks_per_append=blk.n_ticks)
        feed, n = self.ring.last_feed
        self.episode_log.update(feed, n, tick_base=blk.t0)  # (`tick` counts from this run's first tick, also in a log carried over)

    def finish(self) -> EpisodeLog:
        env, metrics, first_record = self.env, self.metrics, self.first_record
        self.finished = True
        _save(self.trainer.models, self.save_dir, "100%")  # train.py:453-457 (written whether or not anything trained, as there)
        # ---- the only read-back: the episode log (records and info counters) and the loss history ----
        rec = self.episode_log.records()
        loss_rows = self.losses.cpu().tolist()
        metrics.set({SusMetrics.AVG_IMPOSTER_RETURNS: rec["imposter_return"][first_record:].tolist(),
                     SusMetrics.AVG_CREW_RETURNS: rec["crew_return"][first_record:].tolist()})
        metrics.set({SusMetrics.IMPOSTER_LOSS: [r[0] for r in loss_rows], SusMetrics.CREW_LOSS: [r[1] for r in loss_rows]})
        if self.per_episode_info:  # the stepping kernels emit the counters where an episode ends (feed["ep_info"])
            metrics.set(info_metric_lists(rec, first_record))
        else:  # one entry per counter: its mean per finished episode over the run, from the env's lifetime accumulators
            life = (env.lifetime_totals() - self.life0).cpu().tolist()
            episodes = life[L.LIFETIME_NAMES.index("episodes")]
            metrics.set({m: [(life[L.LIFETIME_NAMES.index(name)] / max(episodes, 1)) if name else 0.0] for m, name in _LIFETIME_OF.items()})
        return self.episode_log


def _run_blocks(runs: List[_Run], blocks: List[Block], train_step, snapshot_interval=None, stop_after=None, completed: int = 0) -> List[EpisodeLog]:
    """THE block loop: per block every run's ``before_train_step``, then -- where the block ends on a train tick -- ``train_step(k)``, which
    writes row ``k`` of the training runs' loss histories.  ``completed``: the ticks a resumed run has behind it (a block boundary: its
    blocks are skipped).  At the boundaries ``snapshot_boundaries`` / ``stop_boundary`` name every run writes its ``run_state.pt`` -- the
    only place where the loop waits for the device --; at ``stop_after``'s the loop then returns without finishing the runs.  With both
    None no boundary is named and the loop is the one above, launch for launch."""
    snaps = frozenset(snapshot_boundaries(blocks, snapshot_interval)) if snapshot_interval is not None else frozenset()
    stop = stop_boundary(blocks, stop_after) if stop_after is not None else None
    if stop is not None and stop <= completed:
        raise ValueError(f"stop_after = {stop_after} stops at {stop} completed ticks, and the resumed run has {completed} behind it")
    k_train = sum(blk.trains for blk in blocks if blk.t0 < completed)
    for blk in blocks:
        if blk.t0 < completed:
            continue
        for run in runs:
            run.before_train_step(blk)
        if blk.trains:  # train.py:402-416
            train_step(k_train)
            k_train += 1
        done = blk.t0 + blk.n_ticks
        if done == stop or done in snaps:
            for run in runs:  # (a sweep: one file per member directory, all at this boundary)
                run.snapshot(done, k_train)
            if done == stop:
                return [run.episode_log for run in runs]
    return [run.finish() for run in runs]


def _resume_states(who: str, resume_from, n: int, blocks: List[Block]):
    """``resume_from`` of ``train`` (one run directory, or the dict ``read_run_state`` returned) / ``train_sweep`` (a list of them, one per
    member) as ``(states, completed ticks)``; ``([None] * n, 0)`` without one.  The members of a sweep must stand at one boundary."""
    if resume_from is None:
        return [None] * n, 0
    items = list(resume_from) if isinstance(resume_from, (list, tuple)) else [resume_from]
    if len(items) != n:
        raise ValueError(f"{who}: resume_from names {len(items)} run(s), the call has {n}")
    states = [item if isinstance(item, dict) else read_run_state(item) for item in items]
    done = sorted(set(int(s["completed_ticks"]) for s in states))
    if len(done) != 1:
        raise ValueError(f"{who}: the members' snapshots stand at different ticks {done}: a sweep is stopped and resumed as one")
    if done[0] != 0 and done[0] not in [blk.t0 + blk.n_ticks for blk in blocks]:
        raise ValueError(f"{who}: the snapshot stands at {done[0]} completed ticks, which is no block boundary of this schedule")
    return states, done[0]


def train(env, metrics: EpisodicMetricHandler, num_steps: int, replay_buffer: DeviceReplayBuffer, policy: PolicyRollout,
          trainer: DeviceDQNTeamTrainer, scheduler: ExponentialSchedule, save_directory_path, train_step_interval: int = 5,
          batch_size: int = 32, num_saves: int = 5, target_update_interval: int = 10_000, generator: Optional[torch.Generator] = None,
          episode_log: Optional[EpisodeLog] = None, per_episode_info: bool = False, snapshot_interval: Optional[int] = None,
          stop_after: Optional[int] = None, resume_from=None) -> EpisodeLog:
    """``train()`` of src/train.py:284-471.  ``num_steps`` counts lockstep ticks: each adds ``env.batch`` transitions.  ``policy``: the
    ``PolicyRollout`` the teams act by (reference MLPs a network kernel serves -- the fused kernels on the compiled-in layouts, the dense
    kernel on every other game / component set / layer stack, where the learner is ``torch_train_step``; a crew model of None = random crew); ``trainer``: the
    ``DeviceDQNTeamTrainer`` over the same models (built with ``policy=policy``, so that acting follows the trained weights).  ``policy`` may
    also be a ``WindowedPolicyRollout(kernels=True)`` over ``SpatialDQN``s that ``susnet_spatial_forward`` serves, with a trainer built
    ``featurizer=..., spatial=True``: the reference's default model (train.py:152-176);
    ``generator``: draws the replay samples.  ``metrics`` receives what the reference's handler holds after its ``train()``: the teams'
    returns with one entry per episode, the loss per train step, and the nine info counters -- with ``per_episode_info=True`` one entry
    per episode, in episode order (what ``metrics.step(info)`` appends at every episode end, train.py:419-427; ``run_experiment`` asks for
    it); by default ONE entry each, the mean per finished episode over the run.  The ``EpisodeLog`` (returned) keeps tick, env, length, cause
    and info counters of every episode as well.

    Stopping and carrying on (all three None by default: nothing below happens, and the loop is launch for launch the one it was).
    ``snapshot_interval=n``: at the first block boundary at or beyond every ``n`` completed ticks (``snapshot_boundaries``) the run's whole
    state goes to ``save_directory_path/run_state.pt`` -- written under a temporary name, then ``os.replace``d; one file, the latest.
    ``stop_after=t``: the run stops at the first block boundary with at least ``t`` completed ticks (``stop_boundary``), writes the
    snapshot and returns WITHOUT the ``100%`` checkpoints and without filling ``metrics``: it is not finished (the checkpoints and target
    syncs of the completed blocks have happened).  ``resume_from``: the directory of such a snapshot (or the dict ``read_run_state``
    returned).  Build env, models, ring, policy and trainer as for the first call -- any initial weights -- and pass the same arguments:
    there is no ``env.reset()``; the snapshot is loaded into the objects and the loop continues with the first block it has not done, to
    the end an uninterrupted run reaches, bit for bit (the torch learner, ``torch_train_step``, is restored like the others, but its
    kernels are torch's, not pinned here).  Stopping on wall-clock time is not offered: the loop never waits for the device, so the
    host clock says nothing about progress -- choose ``stop_after`` from a measured tick rate."""
    blocks = plan_blocks(num_steps, train_step_interval, target_update_interval, num_saves)
    (state,), completed = _resume_states("train", resume_from, 1, blocks)
    schedule = dict(train_step_interval=int(train_step_interval), batch_size=int(batch_size), num_saves=int(num_saves),
                    target_update_interval=int(target_update_interval))
    run = _Run("train", env, metrics, num_steps, replay_buffer, policy, trainer, scheduler, save_directory_path, blocks, generator, episode_log,
               per_episode_info, schedule, state)

    def train_step(k):
        if run.trains:
            run.losses[k].copy_(trainer.train_step(replay_buffer, batch_size, generator))

    return _run_blocks([run], blocks, train_step, snapshot_interval, stop_after, completed)[0]


def train_sweep(members, num_steps: int, train_step_interval: int = 5, batch_size: int = 32, num_saves: int = 5,
                target_update_interval: int = 10_000, per_episode_info: bool = False, snapshot_interval: Optional[int] = None,
                stop_after: Optional[int] = None, resume_from=None) -> List[EpisodeLog]:
    """``train()`` for the members of a sweep in lockstep -- the reference's loop over ``run_experiment(**config)``
    (notebooks/experiment_1v1.ipynb, notebooks/experiment_mlp.ipynb) with the runs side by side.  ``members``: one
    ``(env, metrics, replay_buffer, policy, trainer, scheduler, save_directory_path, generator)`` per run, each with its own env, ring,
    models and generator.  Per block every member first does what ``train()`` does before the train step -- its saves, its target sync,
    its ``collect`` at its own epsilon, its ``EpisodeLog.update`` -- then ONE ``DeviceDQNSweepTrainer.train_step`` steps all members
    (``susnet_dqn_train_sweep``, or for ``WindowedPolicyRollout(kernels=True)`` members with ``spatial=True`` trainers
    ``susnet_spatial_train_sweep``, or for members with ``dense=True`` trainers off the fused learner's ground
    ``susnet_mlp_train_sweep``: the launches of one learner's step).  The schedule (``num_steps``, ``train_step_interval``,
    ``batch_size``, ``num_saves``, ``target_update_interval``) is shared.  Each member's metrics, losses, checkpoints and ``EpisodeLog``
    (returned, in member order) are what ``train()`` alone produces for it: its step is bitwise its own, and its random streams are
    its own (give every member a generator: without one the draws come from the device's global generator, in member order).
    ``snapshot_interval``, ``stop_after``, ``resume_from`` (the list of the members' run directories, in member order): as in ``train``;
    the sweep is stopped and resumed as one -- every member writes its ``run_state.pt`` into its own directory at the same boundary.
    (A snapshot holds the global generator's state per member; members without a generator of their own are restored in member order.)"""
    members = [tuple(m) for m in members]
    if not members:
        raise ValueError("train_sweep: no members")
    if len(set(id(m[0]) for m in members)) != len(members) or len(set(id(m[2]) for m in members)) != len(members):
        raise ValueError("train_sweep: every member needs its own env and its own replay buffer")
    blocks = plan_blocks(num_steps, train_step_interval, target_update_interval, num_saves)
    states, completed = _resume_states("train_sweep", resume_from, len(members), blocks)
    schedule = dict(train_step_interval=int(train_step_interval), batch_size=int(batch_size), num_saves=int(num_saves),
                    target_update_interval=int(target_update_interval))
    runs = [_Run(f"train_sweep: member {k}", env, metrics, num_steps, ring, policy, trainer, scheduler, save_dir, blocks, generator, None,
                 per_episode_info, schedule, states[k])
            for k, (env, metrics, ring, policy, trainer, scheduler, save_dir, generator) in enumerate(members)]
    training = [run for run in runs if run.trains]  # (a member with no trained team takes no step and draws no sample, as in train())
    sweep = DeviceDQNSweepTrainer([run.trainer for run in training]) if training else None

    def train_step(k):
        if sweep is not None:
            out = sweep.train_step([run.ring for run in training], batch_size, [run.generator for run in training])
            for j, run in enumerate(training):
                run.losses[k].copy_(out[j])

    return _run_blocks(runs, blocks, train_step, snapshot_interval, stop_after, completed)


@dataclasses.dataclass(frozen=True)
class _Settings:
    """What ``run_experiment`` and ``run_sweep`` share of a run's settings; a sweep member's are the shared record with its variant's keys
    replaced.  ``seed`` is a sweep member's (None: ``run_experiment``); ``run_sweep`` has no ``rnn_dropout_seed`` and no
    ``act_dropout_seed``."""
    num_steps: int
    sequence_length: int
    replay_buffer_size: int
    replay_prepopulate_steps: int
    batch_size: int
    gamma: float
    scheduler_start_eps: float
    scheduler_end_eps: float
    scheduler_time_steps: int
    train_imposter: bool
    train_crew: bool
    learning_rate: float
    train_step_interval: int
    num_checkpoint_saves: int
    target_update_interval: int
    dense_train: bool = False
    rnn_dropout_seed: Optional[int] = None
    act_dropout_seed: Optional[int] = None
    seed: Optional[int] = None

    @classmethod
    def of(cls, arguments: dict) -> "_Settings":
        """From an entry point's ``locals()``: the fields it has as parameters, by name."""
        return cls(**{f.name: arguments[f.name] for f in dataclasses.fields(cls) if f.name in arguments})

    def train_keywords(self) -> dict:
        """The schedule as ``train`` / ``train_sweep`` take it."""
        return dict(train_step_interval=self.train_step_interval, batch_size=self.batch_size, num_saves=self.num_checkpoint_saves,
                    target_update_interval=self.target_update_interval, per_episode_info=True)


_Member = namedtuple("_Member", ("env", "metrics", "ring", "policy", "trainer", "scheduler", "directory", "generator", "config"))
_Member.__doc__ = """A run as ``_build_member`` builds it: a member tuple of ``train_sweep``, then the dict ``config.json`` will hold."""


def _experiment_config(env, imposter_model, crew_model, components, base, s: _Settings, featurizer_type=None) -> dict:
    """What ``run_experiment`` writes into ``config.json`` (train.py:185-211), in its key order."""
    return {
        "num_steps": s.num_steps, "batch": env.batch, "imposter_model_args": getattr(imposter_model, "config", None),
        "crew_model_args": getattr(crew_model, "config", None), "imposter_model_type": model_type(imposter_model),
        "crew_model_type": model_type(crew_model), "featurizer_type": featurizer_type or "flat:" + "+".join(components),
        "sequence_length": s.sequence_length, "replay_buffer_size": s.replay_buffer_size, "replay_prepopulate_steps": s.replay_prepopulate_steps,
        "batch_size": s.batch_size, "gamma": s.gamma, "scheduler_start_eps": s.scheduler_start_eps, "scheduler_end_eps": s.scheduler_end_eps,
        "scheduler_time_steps": s.scheduler_time_steps, "train_imposter": s.train_imposter, "train_crew": s.train_crew,
        "experiment_base_dir": str(base), "optimizer_type": "adam", "learning_rate": s.learning_rate,
        "train_step_interval": s.train_step_interval, "target_update_interval": s.target_update_interval,
    }


def spatial_unserved_reason(env, featurizer, model, n_actions: int, T: int) -> Optional[str]:
    """Why ``WindowedPolicyRollout(kernels=True)`` does not act for ``model`` on ``featurizer``'s tensors -- the bound that failed -- or None
    if it does."""
    from .features import GlobalFeaturizer, PerspectiveFeaturizer

    if not isinstance(model, SpatialDQN):
        return f"a SpatialDQN is served, got {type(model).__name__}"
    if not isinstance(featurizer, (GlobalFeaturizer, PerspectiveFeaturizer)) or featurizer.env is not env:
        return "the featurizer must be a GlobalFeaturizer / PerspectiveFeaturizer over the env that is trained on"
    if not 1 <= T <= L.SPATIAL_MAX_T:
        return f"sequence_length = {T}: windows of 1 .. {L.SPATIAL_MAX_T} states are served (SUSNET_SPATIAL_MAX_T)"
    desc = spatial_desc(model)
    if desc is None:
        return ("susnet_spatial_forward does not serve this module: square 1 / 3 / 5 kernels, at most "
                f"{L.SPATIAL_MAX_CONV} convolutions of at most 32 channels on images of at most {L.SPATIAL_MAX_N} x {L.SPATIAL_MAX_N} x "
                f"{L.SPATIAL_MAX_C}, an RNN input of at most {L.SPATIAL_MAX_R}, at most {L.SPATIAL_MAX_RNN_LAYERS} unidirectional tanh RNN layers "
                f"with biases, a Linear + single-slope PReLU head of widths up to {L.MLP_MAX_HIDDEN}")
    return spatial_feed_mismatch(env, featurizer, desc, n_actions)


def _check_spatial_models(who: str, env, featurizer, imposter_model, crew_model, T: int) -> None:
    """``ValueError`` unless ``WindowedPolicyRollout(kernels=True)`` acts for both teams: each present team's ``SpatialDQN`` is served
    (``spatial_unserved_reason``; ``who`` may name a sweep's variant), and a random crew has the production stream (that message names the
    entry point alone, as it always has)."""
    for team, model, n_actions in (("imposter", imposter_model, env.n_imposter_actions), ("crew", crew_model, env.n_crew_actions)):
        if team == "crew" and model is None:
            continue
        why = spatial_unserved_reason(env, featurizer, model, n_actions, T)
        if why is not None:
            raise ValueError(f"{who}: the {team} model is not served by the spatial kernels: {why}")
    if crew_model is None and env.rng_kind != "philox":
        raise ValueError(f"{who.partition(':')[0]}: a random crew draws from the production stream: build the env with rng='philox'")


def _build_member(variant: Optional[int], env, models, components, featurizer, s: _Settings, dirs, generator) -> _Member:
    """THE place a run is built -- ``run_experiment``'s one (``variant`` None) and every member of ``run_sweep`` (``variant``: its index):
    the checks of env and models, then policy, trainer, ring, schedule, metric handler and the ``config.json`` dict.  Nothing is written
    and nothing is collected.  ``models``: (imposter, crew); ``dirs``: (experiment_base_dir, the run's own directory).
    ``featurizer`` None is the flat kind: ``env`` fuses ``ObsConfig('flat', components)``, reference MLPs, ``PolicyRollout``.  A Global /
    Perspective featurizer is the spatial kind: raw uint8 observations, ``SpatialDQN``s, ``WindowedPolicyRollout(kernels=True)``, a trainer
    built ``featurizer=..., spatial=True``; ``components`` is not read, and ``config.json`` also names the learner the run takes
    (``train_step``) and the dropout seed.  What the two callers do differently, on purpose:
    * flat ``run_experiment`` acts and trains through the dense kernels wherever the fused ones do not serve, on windows of T states too;
      a flat sweep member is built for the fused kernels, one state (``dense_train`` alone sends its trainer to the dense step) -- unless
      ``dense_train`` is set and the member reads windows of T > 1 states or the fused kernels do not serve one of its acting models: then
      it is built as ``run_experiment``'s run is, and its ``config.json`` also names the learner it takes (``train_step``);
    * a sweep member's ``config.json`` carries its ``seed``, and its ``generator`` is made here from that seed (``run_experiment`` passes
      its caller's, or None: the device's global generator)."""
    from .features import GlobalFeaturizer

    sweep, who = variant is not None, "run_experiment" if variant is None else "run_sweep"
    (imposter_model, crew_model), (base, experiment_dir), T = models, dirs, s.sequence_length
    if featurizer is None:
        if env.obs_config.mode != "flat" or list(env.obs_config.components) != components:
            raise ValueError(f"{who}: {'env_factory must build' if sweep else 'build'} the env with obs=ObsConfig('flat', components), auto_reset=True")
        if not isinstance(imposter_model, MLP) or not (crew_model is None or isinstance(crew_model, MLP)):
            raise ValueError(f"{who}: served are reference MLPs (a crew model of None acts randomly)")
        # (at sequence_length > 1 a network that is not dense-served is refused here, naming sequence_length and the input width T * F it needs)
        as_run = not sweep or (s.dense_train and T > 1)  # built as run_experiment's run: acting and training through the dense kernels
        policy = PolicyRollout(env, imposter_model, crew_model, components=components, mask_dead=True,
                               **({"dense": True, "sequence_length": T} if as_run else {}))
        if not as_run and s.dense_train and (policy.fused_imposter is None or (crew_model is not None and policy.fused_crew is None)):
            as_run = True  # a dense_train sweep member whose acting models the fused kernels do not serve: collect would refuse it
            policy = PolicyRollout(env, imposter_model, crew_model, components=components, mask_dead=True, dense=True, sequence_length=T)
        learner = {"dense": s.dense_train or T > 1, "sequence_length": T if T > 1 else None} if as_run else {"dense": s.dense_train}
        featurizer_type = None
    else:
        if env.obs_config.mode != "raw" or env.obs_config.dtype != torch.uint8 or not env.auto_reset:
            raise ValueError(f"{who}: with {'featurizer_factory, env_factory must build' if sweep else 'a featurizer, build'} the env with "
                             "obs=ObsConfig('raw', dtype=torch.uint8), auto_reset=True")
        _check_spatial_models(f"{who}: variant {variant}" if sweep else who, env, featurizer, imposter_model, crew_model, T)
        components = []
        policy = WindowedPolicyRollout(env, featurizer, imposter_model, crew_model, sequence_length=T, mask_dead=True, kernels=True,
                                       act_dropout_seed=s.act_dropout_seed)
        learner = {"featurizer": featurizer, "spatial": True, "rnn_dropout_seed": s.rnn_dropout_seed}
        # (a partially observable Perspective featurizer is on record as what it is: "perspective_room" / "perspective_room_mask")
        featurizer_type = "global" if isinstance(featurizer, GlobalFeaturizer) else "perspective" + featurizer.config.mode[len("persp"):]
    trainer = DeviceDQNTeamTrainer(env, imposter_model, crew_model, components, lr=s.learning_rate, gamma=s.gamma, train_imposter=s.train_imposter,
                                   train_crew=s.train_crew, policy=policy, **learner)
    if featurizer is None and T > 1 and any(trainer.trained) and not trainer.dense:
        raise ValueError(f"{who}: sequence_length = {T}: the trained networks are not served by susnet_mlp_train_step on "
                         f"windows of {T} states (needed: reference MLP stacks with a network input of T * F)")
    ring = DeviceReplayBuffer(s.replay_buffer_size, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    config = _experiment_config(env, imposter_model, crew_model, components, base, s, featurizer_type)
    if sweep:  # its seed is on record, and its replay samples are drawn by a generator of its own, seeded with it
        config["seed"] = s.seed
        generator = torch.Generator(device=env.device)
        generator.manual_seed(int(s.seed))
    if featurizer is None and sweep and as_run:
        # which learner the member's own train steps take (run_sweep names the sweep call instead where that serves the training members)
        own = "susnet_dqn_train_step" if trainer.uses_hip(ring) else "susnet_mlp_train_step" if trainer.uses_dense(ring) else "torch_train_step"
        config["train_step"] = own if any(trainer.trained) else None
    if featurizer is not None:
        # which learner the run's train steps take: susnet_spatial_train_step where it serves the trained teams, else torch_train_step
        config["train_step"] = ("susnet_spatial_train_step" if trainer.uses_spatial(ring) else "torch_train_step") if any(trainer.trained) else None
        config["rnn_dropout_seed"] = s.rnn_dropout_seed
        if s.act_dropout_seed is not None:  # (only then: a run without it writes the config.json it always wrote)
            config["act_dropout_seed"] = s.act_dropout_seed
    scheduler = ExponentialSchedule(s.scheduler_start_eps, s.scheduler_end_eps, s.scheduler_time_steps)
    return _Member(env, EpisodicMetricHandler(), ring, policy, trainer, scheduler, experiment_dir, generator, config)


def _start(members: List[_Member], s: _Settings) -> None:
    """Per member: its directory, ``config.json`` (train.py:212-213), then the ring's prepopulation with random ticks."""
    for m in members:
        m.directory.mkdir(parents=True, exist_ok=True)
        (m.directory / "config.json").write_text(json.dumps(m.config, indent=4, default=str))
        if s.replay_prepopulate_steps > 0:
            m.ring.populate_fused(m.env, s.replay_prepopulate_steps)


def _resume(who: str, members: List[_Member]) -> List[dict]:
    """The resume of freshly built members from their directories: every member's ``config.json`` comparison (``check_resume_config``),
    then every member's snapshot (``read_run_state``).  Nothing is written and no object is touched: a refusal leaves all as it was."""
    for m in members:
        check_resume_config(who, m.config, m.directory)
    return [read_run_state(m.directory) for m in members]


def _stops(s: "_Settings", stop_after) -> bool:
    """Whether ``stop_after`` stops a run of these settings before its end (``stop_boundary`` on its block plan)."""
    if stop_after is None:
        return False
    return stop_boundary(plan_blocks(s.num_steps, s.train_step_interval, s.target_update_interval, s.num_checkpoint_saves), stop_after) is not None


def _base_dir(experiment_base_dir) -> pathlib.Path:
    return pathlib.Path(experiment_base_dir) if experiment_base_dir is not None else pathlib.Path.cwd() / "model_registry" / "experiments"


def run_experiment(env, num_steps: int, imposter_model, crew_model, components: Sequence[str], sequence_length: int = 1,
                   replay_buffer_size: int = 100_000, replay_prepopulate_steps: int = 1000, batch_size: int = 32, gamma: float = 0.99,
                   scheduler_start_eps: float = 1.0, scheduler_end_eps: float = 0.05, scheduler_time_steps: int = 1_000_000,
                   train_imposter: bool = True, train_crew: bool = True, experiment_base_dir=None, learning_rate: float = 0.0001,
                   train_step_interval: int = 5, num_checkpoint_saves: int = 5, target_update_interval: int = 10_000,
                   generator: Optional[torch.Generator] = None, episode_log: Optional[EpisodeLog] = None,
                   dense_train: bool = False, featurizer=None, rnn_dropout_seed: Optional[int] = None,
                   act_dropout_seed: Optional[int] = None, snapshot_interval: Optional[int] = None, stop_after: Optional[int] = None,
                   resume_from=None) -> EpisodicMetricHandler:
    """``run_experiment`` of src/train.py:152-281 with the models given as modules: builds ring, policy, trainer and schedule
    (``_build_member``; a run that is refused there has written nothing), writes ``config.json``, pre-populates the ring with
    ``replay_prepopulate_steps`` random ticks, runs ``train()`` (with ``per_episode_info=True``: the nine info
    entries of ``metrics.json`` hold one value per episode, the reference's shape), writes ``metrics.json`` and the checkpoints into ``experiment_base_dir/<timestamp>/`` and returns the metric handler.  ``replay_buffer_size`` counts transitions.
    ``dense_train=True`` (opt-in): the trainer is built with ``dense=True`` -- off the compiled-in layouts the train step is
    ``susnet_mlp_train_step`` instead of the torch loop.  ``sequence_length`` = T > 1 (the reference's default is 2, train.py:160): the
    networks read the flattened window of the last T states, ``T * F`` inputs (dqn.py:86-90); acting, collecting and the train step
    then all go through the dense kernels (the trainer is built ``dense=True`` whatever ``dense_train`` says), and a network that is not
    dense-served at that T is a ``ValueError``.

    ``featurizer``: a ``GlobalFeaturizer`` / ``PerspectiveFeaturizer`` over ``env`` with ``SpatialDQN`` models (the reference's default,
    train.py:152-176; the crew may be None) -- ``env`` is then built ``obs=ObsConfig('raw', torch.uint8), auto_reset=True`` and ``components``
    is not read.  The teams act through ``WindowedPolicyRollout(kernels=True, sequence_length=T)`` (``susnet_spatial_forward`` +
    ``susnet_agent_policy_actions``), the trainer is built ``featurizer=featurizer, spatial=True`` (a trained team
    ``susnet_spatial_train_step`` does not serve takes ``torch_train_step``), the ring has ``trajectory_size=T``; ``config.json`` names
    ``spatial_dqn`` and ``global`` / ``perspective`` and, as ``train_step``, the learner the run takes; the checkpoints are ``<team>_spatial_dqn_<p>.pt``.  A ``SpatialDQN`` the kernels do not
    act for is a ``ValueError`` that says which bound failed.  ``rnn_dropout_seed`` (with ``featurizer``; None: models with dropout between
    their RNN layers train through ``torch_train_step``): the trainer is built with it, so such models -- the reference's own
    ``rnn_layers: 3, rnn_dropout: 0.2`` -- LEARN under the library's dropout masks (``susnet_spatial_train_step_dropout``), online and target
    network.  The seed is written into ``config.json``.  How they ACT follows ``act_dropout_seed`` (with ``featurizer``; without one it is
    a ``ValueError``): None -- such models act in eval mode (put them there with ``model.eval()``: ``susnet_spatial_forward`` is the
    eval-mode forward and refuses a training-mode model with dropout, as before); a seed -- the policy is built with it
    (``WindowedPolicyRollout(kernels=True, act_dropout_seed=...)``), and every acting forward follows its module's mode as torch does: a
    model left in training mode, which is what the reference's never-``eval()``ed models are (train.py:104, 355-381), acts under nn.RNN's
    dropout between its layers (``susnet_spatial_forward_dropout``; net 2 the imposters, net 3 the crew, one mask offset per acting tick),
    a model in ``eval()`` acts without.  The models are left in the mode the caller gave them (the device train step changes no mode),
    and ``config.json`` carries ``act_dropout_seed`` only when it is given.  ``evaluate()`` / ``evaluate_checkpoints()`` stay eval-mode --
    evaluation is greedy play -- and keep refusing a training-mode model; ``run_sweep`` has no such argument, as it has no
    ``rnn_dropout_seed``; torch's own mask stream cannot be reproduced (include/susnet.h).

    ``snapshot_interval`` / ``stop_after`` / ``resume_from`` (all None by default): as in ``train()`` -- ``run_state.pt`` lies in the run's
    directory; a run that ``stop_after`` stops writes neither the ``100%`` checkpoints nor ``metrics.json`` and returns the (empty) handler.
    ``resume_from=<the run's directory>``: build env and models exactly as for the first call (any initial weights) and pass the same
    arguments.  The run is built as always; the ``config.json`` it would write is compared with the directory's on every key but
    ``experiment_base_dir`` (a difference: ``ValueError`` naming key and both values; nothing has been written then); ``config.json``, the
    prepopulation and ``env.reset()`` are skipped, the snapshot is loaded and the run continues IN THAT DIRECTORY with the first block the
    snapshot has not done, and finishes as an uninterrupted run does -- bit for bit on the HIP learners."""
    sequence_length = int(sequence_length)
    if act_dropout_seed is not None and featurizer is None:
        raise ValueError("run_experiment: act_dropout_seed is for SpatialDQN runs (featurizer=...): reference MLPs have no dropout")
    s = _Settings.of(locals())
    base = _base_dir(experiment_base_dir)
    directory = pathlib.Path(resume_from) if resume_from is not None else base / datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
    m = _build_member(None, env, (imposter_model, crew_model), list(components), featurizer, s, (base, directory), generator)
    state = None
    if resume_from is not None:
        (state,) = _resume("run_experiment", [m])
    else:
        _start([m], s)
    train(env, m.metrics, num_steps, m.ring, m.policy, m.trainer, m.scheduler, m.directory, generator=generator, episode_log=episode_log,
          snapshot_interval=snapshot_interval, stop_after=stop_after, resume_from=state, **s.train_keywords())
    if not _stops(s, stop_after):
        m.metrics.save_metrics(save_file_path=m.directory / "metrics.json")
    return m.metrics


SWEEP_VARIANT_KEYS = ("gamma", "learning_rate", "seed", "scheduler_start_eps", "scheduler_end_eps", "scheduler_time_steps", "name")


def check_variants(variants) -> List[dict]:
    """The variants of ``run_sweep`` as a list of dicts; ``ValueError`` for an empty list or a key outside ``SWEEP_VARIANT_KEYS`` (every
    other setting is shared by the members by construction)."""
    variants = [dict(v) for v in variants]
    if not variants:
        raise ValueError("run_sweep: no variants")
    for k, v in enumerate(variants):
        unknown = sorted(set(v) - set(SWEEP_VARIANT_KEYS))
        if unknown:
            raise ValueError(f"run_sweep: variant {k} has {unknown}; a variant may set {list(SWEEP_VARIANT_KEYS)}, everything else is shared")
    return variants


def sweep_member_dirs(base, variants, timestamp: str) -> List[pathlib.Path]:
    """``base/<name or index>/<timestamp>/`` per variant: one reference-shaped experiment directory each (train.py:181-182)."""
    names = [str(v.get("name", k)) for k, v in enumerate(variants)]
    if len(set(names)) != len(names):
        raise ValueError(f"run_sweep: member directory names repeat: {names}")
    return [pathlib.Path(base) / n / timestamp for n in names]


def run_sweep(env_factory, variants, num_steps: int, imposter_model_factory, crew_model_factory, components: Sequence[str],
              sequence_length: int = 1, replay_buffer_size: int = 100_000, replay_prepopulate_steps: int = 1000, batch_size: int = 32,
              gamma: float = 0.99, scheduler_start_eps: float = 1.0, scheduler_end_eps: float = 0.05, scheduler_time_steps: int = 1_000_000,
              train_imposter: bool = True, train_crew: bool = True, experiment_base_dir=None, learning_rate: float = 0.0001,
              train_step_interval: int = 5, num_checkpoint_saves: int = 5, target_update_interval: int = 10_000,
              seed: int = 0, dense_train: bool = False, featurizer_factory=None, snapshot_interval: Optional[int] = None,
              stop_after: Optional[int] = None, resume_from=None) -> List[EpisodicMetricHandler]:
    """The reference's sweeps -- ``for config in configs: run_experiment(**config)`` (notebooks/experiment_1v1.ipynb,
    notebooks/experiment_mlp.ipynb: gamma 0.99 / 0.9 / 0.8 on one game and one MLP) -- as ONE run: the members collect one after another
    and take their train steps together (``train_sweep``).  The shared arguments are ``run_experiment``'s.  ``variants``: one dict per
    member with any of ``gamma``, ``learning_rate``, ``seed``, ``scheduler_start_eps``, ``scheduler_end_eps``, ``scheduler_time_steps``,
    ``name`` (anything else: ``ValueError``); a key left out takes the shared value.  Per member: ``env_factory(seed)`` builds its env,
    ``featurizer_factory(env)`` -- where there is one -- its featurizer, then under ``torch.manual_seed(seed)``
    ``imposter_model_factory(env)`` / ``crew_model_factory(env)`` its models (``crew_model_factory=None``: random crews);
    ``_build_member`` builds the rest as it builds ``run_experiment``'s run, with a sample generator seeded with ``seed`` too.  Each member gets
    ``experiment_base_dir/<name or index>/<timestamp>/`` with ``config.json`` (carrying the variant's values and ``seed``), the
    checkpoints and ``metrics.json`` as ``run_experiment`` writes them, so plotting over one directory per gamma keeps working.  Returns
    the members' metric handlers.  How a member differs from ``run_experiment``'s run:
    * without ``featurizer_factory`` the sweep is MLP-only as it was (a ``SpatialDQN`` is a ``ValueError`` there).  Without ``dense_train``
      a window of one state is served, through the fused kernels: ``sequence_length=1``.  With ``dense_train=True`` a member on a
      compiled-in layout at ``sequence_length=1`` is built and swept as before (``susnet_dqn_train_sweep``); a member that reads windows
      of ``sequence_length`` > 1 states, or one of whose acting models the fused kernels do not serve (another game, feature set or
      layer stack), is built as ``run_experiment`` builds its run -- ``PolicyRollout(dense=True, sequence_length=T)``, a trainer
      ``dense=True, sequence_length=T``, a ring of ``trajectory_size=T``, the same refusal of stacks the dense step does not serve at
      T > 1 -- and its ``config.json`` carries ``train_step``: ``susnet_mlp_train_sweep`` -- one call per chunk of
      ``MLP_SWEEP_MAX_LEARNERS`` -- where that serves the training members, else the member's own learner;
    * with ``featurizer_factory`` (``SpatialDQN`` members, ``sequence_length`` 1 .. ``SPATIAL_MAX_T``) there is no dropout seed
      (``config.json`` says None): members with dropout between their RNN layers take ``torch_train_step`` one after another (a
      ``DeviceDQNSweepTrainer`` over trainers built with ``rnn_dropout_seed`` does sweep them);
    * ``train_step`` in a ``SpatialDQN`` member's ``config.json`` is ``susnet_spatial_train_sweep`` -- one call per chunk of
      ``SPATIAL_SWEEP_MAX_LEARNERS`` -- where that serves the training members, else the member's own learner.

    ``snapshot_interval`` / ``stop_after`` / ``resume_from`` (all None by default): as in ``run_experiment``, for the sweep as one -- every
    member writes ``run_state.pt`` into its own directory at the same boundary.  ``resume_from``: the list of the members' directories in
    variant order, or ONE path ``<experiment_base_dir>/<timestamp>`` that stands for ``<experiment_base_dir>/<name or index>/<timestamp>``
    of every member; the factories are called as for the first call, every member's ``config.json`` is compared before anything is
    loaded."""
    components, variants, spatial = list(components), check_variants(variants), featurizer_factory is not None
    if not spatial and not dense_train and sequence_length != 1:
        raise ValueError("run_sweep: a window of one state is served (sequence_length=1): the Q-network kernel and "
                         "susnet_dqn_train_sweep read one state")
    sequence_length = int(sequence_length)
    shared = _Settings.of(locals())
    base = _base_dir(experiment_base_dir)
    if resume_from is None:
        dirs = sweep_member_dirs(base, variants, datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))
    elif isinstance(resume_from, (list, tuple)):
        dirs = [pathlib.Path(d) for d in resume_from]
        if len(dirs) != len(variants):
            raise ValueError(f"run_sweep: resume_from names {len(dirs)} member directories, the sweep has {len(variants)} variants")
    else:  # <base>/<timestamp>: the members' common base with the timestamp
        dirs = sweep_member_dirs(pathlib.Path(resume_from).parent, variants, pathlib.Path(resume_from).name)
    members = []
    for k, (variant, experiment_dir) in enumerate(zip(variants, dirs)):
        s = dataclasses.replace(shared, **{key: val for key, val in variant.items() if key != "name"})
        # the order of the member's random draws: env by seed, torch.manual_seed(seed), the imposter factory, the crew factory
        env = env_factory(int(s.seed))
        featurizer = featurizer_factory(env) if spatial else None
        torch.manual_seed(int(s.seed))
        models = (imposter_model_factory(env), crew_model_factory(env) if crew_model_factory is not None else None)
        members.append(_build_member(k, env, models, components, featurizer, s, (base, experiment_dir), None))
    if spatial:  # which learner the train steps take: the sweep call where it serves all training members, else each member's own
        training = [m for m in members if any(m.trainer.trained)]
        swept = bool(training) and DeviceDQNSweepTrainer([m.trainer for m in training]).uses_spatial([m.ring for m in training])
        for m in members:
            own = m.config.pop("train_step")  # (put back as the last key, behind seed and rnn_dropout_seed, where it has always stood)
            m.config["train_step"] = "susnet_spatial_train_sweep" if swept and own is not None else own
    elif any("train_step" in m.config for m in members):  # (dense_train members built as run_experiment's run: _build_member)
        training = [m for m in members if any(m.trainer.trained)]
        swept = bool(training) and DeviceDQNSweepTrainer([m.trainer for m in training]).uses_dense([m.ring for m in training])
        for m in members:
            if m.config.get("train_step") is not None and swept:
                m.config["train_step"] = "susnet_mlp_train_sweep"
    states = None
    if resume_from is not None:
        states = _resume("run_sweep", members)
    else:
        _start(members, shared)
    train_sweep([m[:8] for m in members], num_steps, snapshot_interval=snapshot_interval, stop_after=stop_after, resume_from=states,
                **shared.train_keywords())
    if not _stops(shared, stop_after):
        for m in members:
            m.metrics.save_metrics(save_file_path=m.directory / "metrics.json")
    return [m.metrics for m in members]


def _evaluate_blocks(env, actor: BlockActor, n_ticks: int, gamma: float, capacity: Optional[int]) -> dict:
    """The frame of ``evaluate``: reset, an ``EpisodeLog`` and a feed of ``actor.n_block`` ticks, then -- one sequence of the actor's, its
    window filled from the fresh state -- per block ``actor.fill`` and ``EpisodeLog.update``; ONE read-back at the end."""
    n_block = actor.n_block
    env.reset()
    if capacity is None:  # an episode takes at least one tick
        capacity = min(env.batch * max(n_ticks, 1), 1 << 22)
    log = EpisodeLog(env, gamma=gamma, capacity=capacity)
    feed = env.alloc_feed(n_block)
    actor.start(fill_window=True)
    t = 0
    while t < n_ticks:
        n = min(n_block, n_ticks - t)
        actor.fill(feed, n)
        log.update(feed, n, tick_base=t)
        t += n
    if actor.refresh_obs_after:
        env.refresh_obs()  # leave env.obs on the state the last tick produced, as step() does
    return summarize_episodes(log.records(), ticks=n_ticks)


@torch.no_grad()
def evaluate(env, imposter_model, crew_model, components: Sequence[str], n_ticks: int, epsilon: float = 0.0, block_ticks: int = 64,
             mask_dead: bool = True, gamma: float = 1.0, capacity: Optional[int] = None, sequence_length: int = 1, featurizer=None) -> dict:
    """How a pair of models plays: ``env.reset()``, then the acting loop for ``n_ticks`` lockstep ticks in blocks of ``block_ticks``
    (``policy.BlockActor`` fills a feed, as it does for ``DeviceReplayBuffer.collect`` -- one rollout launch per block where the env serves
    it --, + one ``EpisodeLog.update`` per block; no ring, no trainer), and ONE read-back at the end.
    ``crew_model=None``: a random crew.  Returns ``episodes``, ``imposter_win_rate``, ``crew_win_rate``, ``truncation_rate``,
    ``mean_imposter_return``, ``mean_crew_return`` (``gamma``-discounted; 1.0 = plain sums), ``mean_length`` and the mean of every info
    counter per finished episode (``mean_<counter>``), plus ``dropped`` (episodes beyond ``capacity``, not in the means) and ``ticks``.
    Rates and means of zero episodes are NaN.  ``sequence_length`` = T > 1: models that read the window of the last T states (``T * F``
    inputs), acting as in ``DeviceReplayBuffer.collect``: the actor's dense ticks on the policy's feature window, which starts as the fresh
    state T times.  ``featurizer`` (a ``GlobalFeaturizer`` / ``PerspectiveFeaturizer`` over ``env``, which then fuses ``ObsConfig('raw', torch.uint8)``):
    ``SpatialDQN`` models acting as in ``collect`` through ``WindowedPolicyRollout(kernels=True, sequence_length=T)``; ``components`` is not
    read.  Evaluation is greedy play in EVAL mode: there is no ``act_dropout_seed`` here, and a training-mode model with dropout between its
    RNN layers is refused (call ``model.eval()``), whatever ``run_experiment`` acted under."""
    if not env.auto_reset:
        raise ValueError("evaluate: the env must be built with auto_reset=True (episodes restart inside the rollout launch)")
    n_ticks = int(n_ticks)
    n_block = max(1, min(int(block_ticks), n_ticks))
    if featurizer is not None:
        T = int(sequence_length)
        if env.obs_config.mode != "raw" or env.obs_config.dtype != torch.uint8:
            raise ValueError("evaluate: with a featurizer, build the env with obs=ObsConfig('raw', dtype=torch.uint8), auto_reset=True")
        _check_spatial_models("evaluate", env, featurizer, imposter_model, crew_model, T)
        policy = WindowedPolicyRollout(env, featurizer, imposter_model, crew_model, sequence_length=T, epsilon=epsilon, mask_dead=mask_dead, kernels=True)
        return _evaluate_blocks(env, BlockActor(env, policy, epsilon, mask_dead, n_block), n_ticks, gamma, capacity)
    policy = PolicyRollout(env, imposter_model, crew_model, components=list(components), epsilon=epsilon, mask_dead=mask_dead, dense=True,
                           sequence_length=sequence_length)
    actor = BlockActor(env, policy, epsilon, mask_dead, n_block)
    if not actor.imp_served or not actor.crew_served:
        raise ValueError("evaluate: served are reference MLPs a network kernel runs (the compiled-in feature layouts, or the dense kernel); "
                         "a crew model of None acts randomly")
    if actor.kind == "dense":
        check_policy_step_actions("evaluate", env)
        check_random_crew_stream("evaluate", env, policy)
    elif not actor.one_kernel:  # (collect acts tick by tick with such a policy: the network launch(es) + susnet_policy_step)
        raise ValueError("evaluate: this env / model pair / epsilon is not served by the one-kernel policy tick (susnet_qnet_policy_step)")
    return _evaluate_blocks(env, actor, n_ticks, gamma, capacity)


def summarize_episodes(rec, ticks: Optional[int] = None) -> dict:
    """The evaluation summary of ``EpisodeLog.records()`` (a log fed with ``ep_info``): see ``evaluate``."""
    n = int(rec["count"])
    mean = lambda x: float(np.mean(x)) if n else float("nan")
    out = {"episodes": n, "dropped": int(rec["dropped"]), "imposter_win_rate": mean(rec["imposter_won"]), "crew_win_rate": mean(rec["crew_won"]),
           "truncation_rate": mean((rec["ended_by"] & L.EPISODE_TRUNCATED) != 0), "mean_imposter_return": mean(rec["imposter_return"]),
           "mean_crew_return": mean(rec["crew_return"]), "mean_length": mean(rec["length"])}
    for m, name in _RECORD_OF.items():
        if name and name not in ("imposter_won", "crew_won"):
            out[f"mean_{m.value}"] = mean(rec[name])
    if ticks is not None:
        out["ticks"] = int(ticks)
    return out


def evaluate_checkpoints(experiment_dir, env, components: Sequence[str], n_ticks: int, epsilon: float = 0.0, **kw) -> dict:
    """``evaluate`` for every checkpoint pair ``imposter_mlp_<p>.pt`` / ``crew_mlp_<p>.pt`` (or ``imposter_spatial_dqn_<p>.pt`` /
    ``crew_spatial_dqn_<p>.pt``, loaded with ``SpatialDQN.load_from_checkpoint``; pass ``featurizer=...``) that ``run_experiment`` wrote into
    ``experiment_dir`` (a run without a crew model: the imposters against a random crew), as a table ``{<p>: summary}`` in the order of
    training progress (``"0"``, ..., ``"100%"``).  Further keywords go to ``evaluate`` (``sequence_length=T`` for a run trained on
    windows)."""
    d = pathlib.Path(experiment_dir)
    found = {}
    for kind, cls in (("mlp", MLP), ("spatial_dqn", SpatialDQN)):
        for path in d.glob(f"imposter_{kind}_*.pt"):
            found[path.stem[len(f"imposter_{kind}_"):]] = (path, cls)
    if not found:
        raise FileNotFoundError(f"evaluate_checkpoints: no imposter_mlp_<p>.pt / imposter_spatial_dqn_<p>.pt under {d}")
    table = {}
    for p in sorted(found, key=lambda s: float(s.rstrip("%"))):
        path, cls = found[p]
        imp = cls.load_from_checkpoint(path, map_location="cpu").to(env.device)
        crew = None
        for kind, crew_cls in (("mlp", MLP), ("spatial_dqn", SpatialDQN)):
            crew_path = d / f"crew_{kind}_{p}.pt"
            if crew_path.exists():
                crew = crew_cls.load_from_checkpoint(crew_path, map_location="cpu").to(env.device)
                break
        table[p] = evaluate(env, imp, crew, components, n_ticks, epsilon=epsilon, **kw)
    return table
