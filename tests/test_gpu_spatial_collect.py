"""SpatialDQN through collect, train(), run_experiment() and evaluate() on the MI355X: DeviceReplayBuffer.collect with a
WindowedPolicyRollout(kernels=True) against the reference trainer's own rings (tests/golden/spatial_collect/); the policy's acting window
against the ring's carried one; train() against a hand-driven twin of its parts, bit for bit; a batch of 8 against its envs taken alone;
run_experiment / evaluate / evaluate_checkpoints end to end."""
import copy
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

import spatial_collect_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RING_FIELDS = U.RING_FIELDS


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


def raw8(pkg):
    return pkg.ObsConfig("raw", dtype=torch.uint8)


def base_1v3(pkg, batch, seed=3, **kw):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9, obs=raw8(pkg),
                                  max_time_steps=kw.pop("max_time_steps", 6), **kw)


NET = dict(strides=[1], paddings=[1], kernel_size=[3, 3], dilations=[1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[12])


def global_models(pkg, env, seeds=(3, 4), crew=True):
    """Small SpatialDQNs on the Global featurizer's tensors of ``env``: two 3x3 convolutions of 6 channels, one RNN layer of 16, one hidden
    layer of 12."""
    A = env.n_agents
    _, planes, non = env._make_obs(pkg.ObsConfig("planes"), 1, rows=1)
    cfg = dict(NET, input_image_size=planes.shape[-1], non_spatial_input_size=non.shape[-1] + A, n_channels=[planes.shape[-3], 6])
    out = []
    for seed, n in zip(seeds, (env.n_imposter_actions, env.n_crew_actions)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            out.append(pkg.SpatialDQN(**cfg, n_actions=n).to(DEV))
    return out[0], (out[1] if crew else None)


def env_from_meta(pkg, meta, batch, **kw):
    grid = np.array(meta["grid_used"], dtype=bool)
    return pkg.BatchedFourRoomEnv(**dict(meta["kwargs"]), grid=grid, batch=batch, **kw)


# ---- 5. the reference trainer's own rings ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.CASES)
def test_spatial_collection_matches_the_reference_trainer_loop(pkg, name):
    """tests/golden/generate_collect_spatial.py: train.py:316-322, 345-399, 419-449 around the unmodified env, featurizer, SpatialDQNs and
    ReplayBuffer; one env, numpy's words as the tape, the stored parameters, greedy."""
    g = U.load_case(name)
    meta = g["meta"]
    T, max_size, num_steps = meta["trajectory_size"], meta["max_size"], meta["num_steps"]
    env = env_from_meta(pkg, meta, 1, device=DEV, rng="numpy", tape_words=1 << 16, auto_reset=True, check_errors=False, obs=raw8(pkg))
    env._reseed([meta["seed"]])
    models = []
    for team in ("imposter", "crew"):
        m = pkg.SpatialDQN(**meta["config"], n_actions=meta["n_actions"][team])
        m.load_state_dict({k[len(team) + 2:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(team + "::")})
        models.append(m.to(DEV).eval())
    featurizer = getattr(pkg.features, meta["featurizer"])(env)
    policy = pkg.WindowedPolicyRollout(env, featurizer, *models, sequence_length=T, mask_dead=True, kernels=True)
    assert policy.spatial_imposter is not None and policy.spatial_crew is not None and policy.sequence_length == T
    assert pkg.policy.served_by_kernels(policy) == (True, True, False) and pkg.policy.acts_per_agent(policy)
    buf = pkg.DeviceReplayBuffer(max_size, meta["state_size"], T, meta["n_agents"], meta["n_imposters"], device=env.device)
    env.reset()
    taken = []
    for part in (37, num_steps - 37):  # two calls: the windows carry over
        assert buf.collect(env, policy, part, epsilon=0.0, mask_dead=True, ticks_per_append=50) == part
        feed, n = buf.last_feed
        taken.append(feed["actions"][:n].clone())
    torch.cuda.synchronize()
    env.poll_errors()
    # the last block of each call, as the reference took them
    np.testing.assert_array_equal(np_(taken[0])[:, 0], g["taken"][:37][-np_(taken[0]).shape[0]:])
    np.testing.assert_array_equal(np_(taken[1])[:, 0], g["taken"][-np_(taken[1]).shape[0]:])
    assert (buf.idx, buf.size) == (meta["idx"], meta["size"])
    n = buf.size
    np.testing.assert_array_equal(np_(buf.actions[:n]), g["actions"].astype(np.int64), err_msg="actions (the networks' greedy choices)")
    np.testing.assert_array_equal(np_(buf.states[:n]), g["states"].astype(np.float32), err_msg="states")
    np.testing.assert_array_equal(np_(buf.next_states[:n]), g["next_states"].astype(np.float32), err_msg="next_states")
    assert np_(buf.rewards[:n]).view(np.uint32).tolist() == g["rewards"].view(np.uint32).tolist(), "rewards"
    np.testing.assert_array_equal(np_(buf.dones[:n]), g["dones"].astype(bool), err_msg="dones")
    np.testing.assert_array_equal(np_(buf.imposters[:n]), g["imposters"], err_msg="imposters")
    # the policy's acting window, moved on from the last slot, is the ring's carried window
    policy.push(feed["done"][n_last(buf)], feed["truncated"][n_last(buf)], feed["obs"][n_last(buf)])
    np.testing.assert_array_equal(np_(policy.window), np_(buf._collect_window))


def n_last(buf):
    return buf.last_feed[1] - 1


# ---- 4c. the acting window follows the carried one --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3])
def test_acting_window_equals_the_carried_window_after_collect(pkg, T):
    env = base_1v3(pkg, 70, seed=9)
    imp, crew = global_models(pkg, env)
    policy = pkg.WindowedPolicyRollout(env, pkg.GlobalFeaturizer(env), imp, crew, sequence_length=T, kernels=True)
    ring = pkg.DeviceReplayBuffer(70 * 7, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    env.reset()
    ring.collect(env, policy, 7, epsilon=0.3, ticks_per_append=3)
    feed, n = ring.last_feed
    assert n == 1  # 3 + 3 + 1
    # the acting window stands one push behind the carried one: it acted on the state before the last tick
    assert policy.window.data_ptr() != ring._collect_window.data_ptr()
    policy.push(feed["done"][n - 1], feed["truncated"][n - 1], feed["obs"][n - 1])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np_(policy.window), np_(ring._collect_window))
    np.testing.assert_array_equal(np_(policy.window[:, -1]), np_(feed["obs"][n - 1]))
    np.testing.assert_array_equal(np_(env.obs), np_(feed["obs"][n - 1]))  # env.obs is left on the state the last tick produced
    assert ring.size == 70 * 7
    # another window length is refused, a policy without kernels too
    with pytest.raises(AssertionError, match="trajectory_size"):
        pkg.DeviceReplayBuffer(64, env.flattened_state_size, T + 1, env.n_agents, env.n_imposters, device=env.device).collect(env, policy, 1)
    eager = pkg.WindowedPolicyRollout(env, pkg.GlobalFeaturizer(env), imp, crew, sequence_length=T, kernels=False)
    with pytest.raises(AssertionError, match="WindowedPolicyRollout\\(kernels=True\\)"):
        ring.collect(env, eager, 1)


# ---- 6. the loop equals its parts --------------------------------------------------------------------------------------------------------
class Greedy:
    def value(self, step):
        return 0.0


def _spatial_setup(pkg, models=None, batch=8, T=2, seed=5, crew=True, lr=1e-3, gamma=0.9, **env_kw):
    env = base_1v3(pkg, batch, seed=seed, **env_kw)
    imp, crew_m = global_models(pkg, env, crew=crew) if models is None else (copy.deepcopy(models[0]), copy.deepcopy(models[1]))
    featurizer = pkg.GlobalFeaturizer(env)
    policy = pkg.WindowedPolicyRollout(env, featurizer, imp, crew_m, sequence_length=T, mask_dead=True, kernels=True)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew_m, [], lr=lr, gamma=gamma, policy=policy, featurizer=featurizer, spatial=True)
    ring = pkg.DeviceReplayBuffer(batch * 9, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)  # (wraps in 11 ticks)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(77)
    return env, (imp, crew_m), policy, trainer, ring, gen


def test_train_equals_collect_and_train_step_in_plan_blocks_order(pkg, tmp_path):
    num_steps, k, u, batch_size, num_saves = 11, 5, 4, 16, 5
    env, models, policy, trainer, ring, gen = _spatial_setup(pkg)
    assert trainer.uses_spatial(ring) and trainer._policy_image(0) is None and trainer._policy_image(1) is None
    initial = (copy.deepcopy(models[0]), copy.deepcopy(models[1]))
    feeds = []
    collect = ring.collect

    def recording_collect(*a, **kw):
        out = collect(*a, **kw)
        feed, n = ring.last_feed
        feeds.append({f: feed[f][:n].clone() for f in ("actions", "rewards", "done", "truncated", "obs", "term_obs", "roles", "ep_info")})
        return out

    ring.collect = recording_collect
    metrics = pkg.EpisodicMetricHandler()
    pkg.train(env, metrics, num_steps, ring, policy, trainer, Greedy(), tmp_path / "run", train_step_interval=k, batch_size=batch_size,
              num_saves=num_saves, target_update_interval=u, generator=gen)
    torch.cuda.synchronize()

    env2, models2, policy2, trainer2, ring2, gen2 = _spatial_setup(pkg, models=initial)
    env2.reset()  # train.py:316
    feeds2, losses2 = [], []
    blocks = pkg.plan_blocks(num_steps, k, u, num_saves)
    for blk in blocks:
        if blk.sync_ticks:
            trainer2.sync_targets()
        ring2.collect(env2, policy2, blk.n_ticks, epsilon=0.0, ticks_per_append=blk.n_ticks)
        feed, n = ring2.last_feed
        assert n == blk.n_ticks
        feeds2.append({f: feed[f][:n].clone() for f in feeds[0]})
        if blk.trains:
            losses2.append(trainer2.train_step(ring2, batch_size, gen2))
    torch.cuda.synchronize()
    assert len(feeds) == len(feeds2) == len(blocks)
    for i, (x, y) in enumerate(zip(feeds, feeds2)):
        for f in x:
            assert torch.equal(x[f], y[f]), f"block {i} feed.{f}"
    assert (ring.idx, ring.size) == (ring2.idx, ring2.size) and ring.size == ring.max_size
    for f in RING_FIELDS:
        assert torch.equal(getattr(ring, f), getattr(ring2, f)), f"ring.{f}"
    for tm in range(2):
        assert trainer.trained[tm]
        assert torch.equal(trainer.flat[tm], trainer2.flat[tm]), f"team {tm} parameters"
        assert torch.equal(trainer.target_flat[tm], trainer2.target_flat[tm]), f"team {tm} target parameters"
        for a, b in zip(trainer.state_tensors(tm), trainer2.state_tensors(tm)):
            assert torch.equal(a, b), f"team {tm} Adam state"
        assert any(not torch.equal(p, q) for p, q in zip(models[tm].parameters(), initial[tm].parameters())), "the team trained"
    want = torch.stack(losses2).cpu().tolist()
    n_train = sum(b.trains for b in blocks)
    assert len(want) == n_train == 1 + (num_steps - 1) // k
    assert metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS] == [r[0] for r in want]
    assert metrics.metrics[pkg.SusMetrics.CREW_LOSS] == [r[1] for r in want]
    assert all(math.isfinite(v) and v > 0 for r in want for v in r)
    names = sorted(os.listdir(tmp_path / "run"))
    pcts = sorted({str(int(t * 100 / num_steps)) for t in pkg.train_loop.save_ticks(num_steps, num_saves)} | {"100%"})
    assert names == sorted(f"{team}_spatial_dqn_{p}.pt" for team in ("imposter", "crew") for p in pcts)
    loaded = pkg.SpatialDQN.load_from_checkpoint(tmp_path / "run" / "imposter_spatial_dqn_100%.pt", map_location="cpu")
    for p, q in zip(loaded.parameters(), models[0].parameters()):
        assert torch.equal(p, q.detach().cpu())


def test_a_batch_of_eight_collects_what_its_envs_collect_alone(pkg):
    """Env b of a batch draws from counter env_id_base + b of the handle's Philox key: a batch-1 env with env_id_base = b is that env."""
    Bn, ticks, T = 8, 9, 2
    env, models, policy, _, _, _ = _spatial_setup(pkg, batch=Bn, seed=21)
    ring = pkg.DeviceReplayBuffer(Bn * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    env.reset()
    ring.collect(env, policy, ticks, epsilon=0.3, ticks_per_append=4)
    torch.cuda.synchronize()
    for b in range(Bn):
        one = base_1v3(pkg, 1, seed=21, env_id_base=b)
        p1 = pkg.WindowedPolicyRollout(one, pkg.GlobalFeaturizer(one), models[0], models[1], sequence_length=T, mask_dead=True, kernels=True)
        r1 = pkg.DeviceReplayBuffer(ticks, one.flattened_state_size, T, one.n_agents, one.n_imposters, device=one.device)
        one.reset()
        r1.collect(one, p1, ticks, epsilon=0.3, ticks_per_append=4)
        torch.cuda.synchronize()
        for f in RING_FIELDS:
            assert torch.equal(getattr(ring, f)[b::Bn], getattr(r1, f)), f"env {b} ring.{f}"


# ---- 7. run_experiment, evaluate, evaluate_checkpoints -------------------------------------------------------------------------------------
@pytest.mark.parametrize("crew", [True, False])
def test_run_experiment_and_evaluate_checkpoints_with_spatial_dqn(pkg, tmp_path, crew):
    env = base_1v3(pkg, 16, seed=7)
    imp, crew_m = global_models(pkg, env, crew=crew)
    featurizer = pkg.GlobalFeaturizer(env)
    num_steps, k = 7, 5
    metrics = pkg.run_experiment(env, num_steps=num_steps, imposter_model=imp, crew_model=crew_m, components=[], sequence_length=2,
                                 replay_buffer_size=500, replay_prepopulate_steps=4, batch_size=8, gamma=0.9, scheduler_time_steps=5,
                                 experiment_base_dir=tmp_path, learning_rate=1e-3, train_step_interval=k, target_update_interval=4,
                                 featurizer=featurizer)
    m = metrics.metrics
    assert len(m[pkg.SusMetrics.IMPOSTER_LOSS]) == 1 + (num_steps - 1) // k
    n_ep = len(m[pkg.SusMetrics.AVG_IMPOSTER_RETURNS])
    assert n_ep >= env.batch  # max_time_steps = 6: every env finishes an episode in 7 ticks
    assert len(m[pkg.SusMetrics.TOTAL_TIME_STEPS]) == n_ep  # per-episode lists, the reference's shape
    (run_dir,) = list(tmp_path.iterdir())
    config = json.loads((run_dir / "config.json").read_text())
    assert config["imposter_model_type"] == "spatial_dqn" and config["crew_model_type"] == ("spatial_dqn" if crew else "random")
    assert config["featurizer_type"] == "global" and config["sequence_length"] == 2
    assert config["imposter_model_args"] == json.loads(json.dumps(imp.config)) and (config["crew_model_args"] is None) == (not crew)
    assert config["train_step"] == "susnet_spatial_train_step"  # trainer.uses_spatial(ring)
    saved = json.loads((run_dir / "metrics.json").read_text())
    assert saved["avg_imposter_returns"] == m[pkg.SusMetrics.AVG_IMPOSTER_RETURNS]
    written = sorted(p.name for p in run_dir.glob("imposter_spatial_dqn_*.pt"))
    assert "imposter_spatial_dqn_100%.pt" in written and "imposter_spatial_dqn_0.pt" in written
    assert (run_dir / "crew_spatial_dqn_100%.pt").exists() == crew
    table = pkg.train_loop.evaluate_checkpoints(run_dir, env, [], 8, featurizer=featurizer, sequence_length=2, block_ticks=3)
    assert sorted(table) == sorted(n[len("imposter_spatial_dqn_"):-3] for n in written)
    assert all(s["ticks"] == 8 and s["episodes"] >= env.batch for s in table.values())


def test_evaluate_equals_a_hand_fed_episode_log(pkg):
    env = base_1v3(pkg, 16, seed=13)
    imp, crew_m = global_models(pkg, env)
    featurizer = pkg.GlobalFeaturizer(env)
    n_ticks, T = 10, 2
    got = pkg.evaluate(env, imp, crew_m, [], n_ticks, epsilon=0.2, block_ticks=4, gamma=0.9, sequence_length=T, featurizer=featurizer)
    # by hand on a twin: the same acting loop in the same blocks
    env2 = base_1v3(pkg, 16, seed=13)
    policy = pkg.WindowedPolicyRollout(env2, pkg.GlobalFeaturizer(env2), imp, crew_m, sequence_length=T, mask_dead=True, kernels=True)
    env2.reset()
    log = pkg.EpisodeLog(env2, gamma=0.9, capacity=16 * n_ticks)
    feed = env2.alloc_feed(4)
    policy.reset_window()
    last = None
    for t0 in range(0, n_ticks, 4):
        n = min(4, n_ticks - t0)
        for k in range(n):
            if last is not None:
                policy.push(feed["done"][last], feed["truncated"][last], feed["obs"][last])
            q_imp, q_crew = policy.q_rows()
            env2.agent_policy_tick_into(feed, k, q_imp, q_crew, epsilon=0.2, mask_dead=True)
            last = k
        log.update(feed, n, tick_base=t0)
    want = pkg.train_loop.summarize_episodes(log.records(), ticks=n_ticks)
    assert got["episodes"] >= 16 and set(got) == set(want)
    for key in want:
        assert got[key] == want[key] or (math.isnan(got[key]) and math.isnan(want[key])), key


def test_run_experiment_says_which_bound_failed(pkg, tmp_path):
    env = base_1v3(pkg, 4, seed=2)
    imp, crew_m = global_models(pkg, env)
    with pytest.raises(ValueError, match="sequence_length = 9"):
        pkg.run_experiment(env, 4, imp, crew_m, [], sequence_length=9, experiment_base_dir=tmp_path, featurizer=pkg.GlobalFeaturizer(env))
    with pytest.raises(ValueError, match="non-spatial width"):  # a Global network on the Perspective featurizer's tensors
        pkg.run_experiment(env, 4, imp, crew_m, [], sequence_length=2, experiment_base_dir=tmp_path, featurizer=pkg.PerspectiveFeaturizer(env))
    with pytest.raises(ValueError, match="a SpatialDQN is served"):
        pkg.run_experiment(env, 4, pkg.MLP([4, 4, env.n_imposter_actions]), None, [], sequence_length=2, experiment_base_dir=tmp_path,
                           featurizer=pkg.GlobalFeaturizer(env))
    assert not list(tmp_path.iterdir())  # refused before anything is written
    # the MLP path keeps its refusals and their wording
    with pytest.raises(ValueError, match="ObsConfig\\('flat'"):
        pkg.run_experiment(env, 4, imp, crew_m, ["onehot_pos"], experiment_base_dir=tmp_path)
