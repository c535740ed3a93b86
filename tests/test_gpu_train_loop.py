"""train() / run_experiment() on the MI355X: the block loop against a hand-written per-tick sequence of the primitives it is made of
(collect, train_step, sync_targets) in the reference's order (src/train.py:328-416), bitwise."""
import copy
import importlib
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_fixtures as ef  # noqa: E402

pytestmark = pytest.mark.gpu

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _game(pkg, game, batch=256, seed=5):
    if game == "1v2":
        comps = COMPS3
        env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=14,
                                     shuffle_imposter_index=True, max_time_steps=30, obs=pkg.ObsConfig("flat", comps))
    else:
        comps = ["onehot_pos"]
        kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
        env = pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device="cuda:0", rng="philox", seed=seed,
                                                auto_reset=True, obs=pkg.ObsConfig("flat", comps))
    return env, comps


def _setup(pkg, game, models=None, lr=1e-3, gamma=0.9, ring_rows=256 * 24):
    env, comps = _game(pkg, game)
    if models is None:
        imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
        crew = pkg.policy.reference_crew_mlp(env, comps, seed=4) if game == "1v2" else None
    else:
        imp, crew = copy.deepcopy(models[0]), copy.deepcopy(models[1])
    policy = pkg.PolicyRollout(env, imp, crew, components=comps, mask_dead=True)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew, comps, lr=lr, gamma=gamma, policy=policy)
    ring = pkg.DeviceReplayBuffer(ring_rows, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)  # (wraps during the run)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(77)
    return env, comps, (imp, crew), policy, trainer, ring, gen


@pytest.mark.parametrize("game", ["1v1", "1v2"])
def test_train_equals_the_per_tick_sequence_of_its_primitives(pkg, game, tmp_path):
    num_steps, k, u, batch_size, num_saves = 41, 3, 7, 64, 5
    sched = pkg.ExponentialSchedule(1.0, 0.05, 30)

    # ---- train() ----
    env, comps, models, policy, trainer, ring, gen = _setup(pkg, game)
    assert trainer.hip and policy.fused_imposter is not None
    initial = (copy.deepcopy(models[0]), copy.deepcopy(models[1]))
    env.reset()
    life0 = env.lifetime_totals().clone()
    metrics = pkg.EpisodicMetricHandler()
    log = pkg.train(env, metrics, num_steps, ring, policy, trainer, sched, tmp_path / "run", train_step_interval=k, batch_size=batch_size,
                    num_saves=num_saves, target_update_interval=u, generator=gen)
    torch.cuda.synchronize()
    episodes = int((env.lifetime_totals() - life0)[pkg._lib.LIFETIME_NAMES.index("episodes")])

    # ---- the same run tick by tick, in the reference's order: sync, act + step + add, train ----
    env2, _, models2, policy2, trainer2, ring2, gen2 = _setup(pkg, game, models=initial)
    for a, b in zip(trainer.flat, trainer2.flat):
        assert (a is None) == (b is None)
    env2.reset()
    env2.reset()  # (as above: once before the lifetime totals are read, once by train() itself, train.py:316)
    step_losses, ticks = [], {f: [] for f in ("rewards", "done", "truncated", "roles")}
    for t in range(num_steps):
        if t % u == 0:
            trainer2.sync_targets()
        block_first = 0 if t == 0 else ((t - 1) // k) * k + 1  # (epsilon is one value per block: the documented deviation)
        ring2.collect(env2, policy2, 1, epsilon=float(sched.value(block_first)), ticks_per_append=1)
        feed, n = ring2.last_feed
        assert n == 1
        for f in ticks:
            ticks[f].append(feed[f][0].clone())
        if t % k == 0:
            step_losses.append(trainer2.train_step(ring2, batch_size, gen2))
    torch.cuda.synchronize()

    assert (ring.idx, ring.size) == (ring2.idx, ring2.size) and ring.size == ring.max_size
    for f in RING_FIELDS:
        assert torch.equal(getattr(ring, f), getattr(ring2, f)), f"ring.{f}"
    for tm in range(2):
        if not trainer.trained[tm]:
            assert trainer2.flat[tm] is None
            continue
        assert torch.equal(trainer.flat[tm], trainer2.flat[tm]), f"team {tm} parameters"
        assert torch.equal(trainer.target_flat[tm], trainer2.target_flat[tm]), f"team {tm} target parameters"
        for a, b in zip(trainer.state_tensors(tm), trainer2.state_tensors(tm)):
            assert torch.equal(a, b), f"team {tm} Adam state"
        assert not torch.equal(trainer.flat[tm], trainer.target_flat[tm])  # (41 ticks: trained after the last sync at tick 35)
    # the loss history is the per-step tensors
    n_train = 1 + (num_steps - 1) // k
    want_losses = torch.stack(step_losses).cpu().tolist()
    assert len(want_losses) == n_train
    assert metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS] == [r[0] for r in want_losses]
    assert metrics.metrics[pkg.SusMetrics.CREW_LOSS] == [r[1] for r in want_losses]
    assert any(v > 0 for v in metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS])
    # the episode log is the numpy path on the same ticks, and holds one record per episode the env finished
    host_feed = {f: torch.stack(v).cpu().numpy() for f, v in ticks.items()}
    host = pkg.EpisodeLog(gamma=trainer.gamma, capacity=1 << 16, n_agents=env.n_agents, batch=env.batch)
    for blk in pkg.plan_blocks(num_steps, k, u, num_saves):
        host.update(ef.slice_feed(host_feed, blk.t0, blk.t0 + blk.n_ticks))
    got, want = log.records(), host.records()
    ef.assert_records_equal(got, want)
    assert got["count"] == episodes > 0 and got["dropped"] == 0
    assert metrics.metrics[pkg.SusMetrics.AVG_IMPOSTER_RETURNS] == want["imposter_return"].tolist()
    assert metrics.metrics[pkg.SusMetrics.AVG_CREW_RETURNS] == want["crew_return"].tolist()
    assert metrics.metrics[pkg.SusMetrics.TOTAL_TIME_STEPS] == [float(want["length"].sum()) / episodes]
    assert all(math.isfinite(v) for v in metrics.compute().values())
    # checkpoints under the reference's names (train.py:333-338, 453-457), loadable, the last one = the trained weights
    teams = ["imposter"] + (["crew"] if models[1] is not None else [])
    for team in teams:
        for pct in ("0", "24", "48", "73", "100%"):  # t_saves = linspace(0, 41, 4, endpoint=False) = 0, 10, 20, 30
            path = tmp_path / "run" / f"{team}_mlp_{pct}.pt"
            assert path.exists(), sorted(os.listdir(tmp_path / "run"))
            loaded = pkg.MLP.load_from_checkpoint(path, map_location="cpu")
        final = trainer.models[teams.index(team)]
        for p, q in zip(loaded.parameters(), final.parameters()):
            assert torch.equal(p, q.detach().cpu())
    first = pkg.MLP.load_from_checkpoint(tmp_path / "run" / "imposter_mlp_0.pt", map_location="cpu")
    for p, q in zip(first.parameters(), initial[0].parameters()):
        assert torch.equal(p, q.detach().cpu())
    assert len(os.listdir(tmp_path / "run")) == 5 * len(teams)


def test_run_experiment_smoke(pkg, tmp_path):
    env, comps = _game(pkg, "1v2")
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    crew = pkg.policy.reference_crew_mlp(env, comps, seed=4)
    num_steps, k = 64, 5
    metrics = pkg.run_experiment(env, num_steps=num_steps, imposter_model=imp, crew_model=crew, components=comps, replay_buffer_size=50_000,
                                 replay_prepopulate_steps=16, batch_size=32, gamma=0.9, scheduler_time_steps=40, experiment_base_dir=tmp_path,
                                 learning_rate=1e-3, train_step_interval=k, target_update_interval=16)
    m = metrics.metrics
    n_train = 1 + (num_steps - 1) // k
    assert len(m[pkg.SusMetrics.IMPOSTER_LOSS]) == len(m[pkg.SusMetrics.CREW_LOSS]) == n_train
    n_ep = len(m[pkg.SusMetrics.AVG_IMPOSTER_RETURNS])
    assert n_ep == len(m[pkg.SusMetrics.AVG_CREW_RETURNS]) >= env.batch  # (max_time_steps = 30: every env finishes two episodes in 64 ticks)
    assert all(math.isfinite(v) for v in metrics.compute().values())
    (run_dir,) = list(tmp_path.iterdir())
    config = json.loads((run_dir / "config.json").read_text())
    assert config["num_steps"] == num_steps and config["train_step_interval"] == k and config["imposter_model_type"] == "mlp"
    saved = json.loads((run_dir / "metrics.json").read_text())
    assert saved["avg_imposter_returns"] == m[pkg.SusMetrics.AVG_IMPOSTER_RETURNS]
    assert (run_dir / "imposter_mlp_100%.pt").exists() and (run_dir / "crew_mlp_100%.pt").exists()


def test_train_refuses_what_collect_does_not_serve(pkg, tmp_path):
    env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device="cuda:0", rng="philox", seed=1, auto_reset=False, grid_size=14,
                                 obs=pkg.ObsConfig("flat", COMPS3))
    imp = pkg.policy.reference_imposter_mlp(env, COMPS3, seed=3)
    policy = pkg.PolicyRollout(env, imp, None, components=COMPS3)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, None, COMPS3, lr=1e-3, gamma=0.9, policy=policy)
    ring = pkg.DeviceReplayBuffer(1024, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    with pytest.raises(ValueError, match="auto_reset"):
        pkg.train(env, pkg.EpisodicMetricHandler(), 4, ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.1, 10), tmp_path)
    with pytest.raises(ValueError, match="reference MLPs"):
        pkg.run_experiment(env, 4, pkg.RandomEquiprobable(7), None, COMPS3, experiment_base_dir=tmp_path)
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.run_experiment(env, 4, imp, None, COMPS3, sequence_length=2, experiment_base_dir=tmp_path)
