"""The SpatialDQN sweep step (susnet_spatial_train_sweep, DeviceDQNSweepTrainer over spatial members, train_sweep, run_sweep) on the
MI355X.  The oracle throughout is the single-learner step (susnet_spatial_train_step / _dropout), which tests/test_gpu_spatial_train.py and
tests/test_gpu_spatial_dropout.py pin to float64 references: every comparison here is byte for byte, so there is no tolerance."""
import copy
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

from spatial_sweep_util import SweepCall, dropout_step, dropout_workspace, make_drop, same_bits
from spatial_train_util import SpatialCall, as_global, flat, make_batch, make_model
from test_gpu_spatial_train import A3, C3, N5, RAGGED, _game_1v2, _nets, _trainer_models
from train_exact import DEV

pytestmark = pytest.mark.gpu

GAMMAS, LRS = (0.99, 0.9, 0.8), (1e-3, 3e-3, 1e-4)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env3(pkg):
    """A 3-agent, one-imposter handle: the calls take the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


def _learners(pkg, env3, case, layout, K, seed=0, edit=None):
    """K learners of RAGGED ``case``'s shape, each with its own weights, batch, indices, gamma and lr -- built twice from the same seeds:
    the sweep's calls and their twins."""
    n, T, Fn, imp, crew = case
    out = []
    for _ in range(2):
        calls = []
        for k in range(K):
            rng = np.random.default_rng(1000 * seed + 17 * k + n)
            models = _nets(pkg, Fn, (imp, crew), seed=100 * seed + 10 * k + 1)
            batch = make_batch(rng, n, T, A3, C3, N5, Fn, 4)
            if edit is not None:
                edit(k, batch)
            if layout == "global":
                batch = as_global(batch)
            calls.append(SpatialCall(pkg, env3, models, models, batch, GAMMAS[k % 3], lr=LRS[k % 3]))
        out.append(calls)
    return out


# ---- 1. bitwise the single step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["global", "perspective"])
@pytest.mark.parametrize("case", RAGGED[1:3], ids=[f"n{c[0]}-T{c[1]}-Fn{c[2]}" for c in RAGGED[1:3]])
def test_sweep_is_bitwise_the_single_step(pkg, env3, case, layout):
    calls, twins = _learners(pkg, env3, case, layout, 3)
    sweep = SweepCall(pkg, env3, calls)
    for step in range(2):
        got = sweep.step()
        for k, twin in enumerate(twins):
            same_bits(got[k], twin.step(), f"step {step} learner {k}")
    assert all(got[k][1][t]["step"] > 0 for k in range(3) for t in range(2))
    assert not np.array_equal(got[0][1][0]["bits"][0], got[1][1][0]["bits"][0]), "the learners are different learners"


# ---- 2. ragged learners ----------------------------------------------------------------------------------------------------------------------
def test_ragged_learners_skip_their_empty_updates(pkg, env3):
    """Learner 0 has no imposter rows for agent 0, learner 1 only done rows, learner 2 is ordinary."""
    def edit(k, batch):
        if k == 0:
            batch["imposters"] = (1 + np.arange(len(batch["imposters"])) % 2).astype(np.int16)
        if k == 1:
            batch["dones"][:] = 1

    calls, twins = _learners(pkg, env3, RAGGED[2], "perspective", 3, seed=2, edit=edit)
    got = SweepCall(pkg, env3, calls).step()
    for k, twin in enumerate(twins):
        same_bits(got[k], twin.step(), f"learner {k}")
    assert got[0][1][0]["step"] == 2.0 and got[0][1][1]["step"] == 3.0  # (agent 0 is never the imposter: that update did not advance the count)
    assert got[2][1][0]["step"] == 3.0


# ---- 3. the limits -----------------------------------------------------------------------------------------------------------------------------
def test_max_learners_at_the_smallest_batch(pkg, env3):
    K = pkg._lib.SPATIAL_SWEEP_MAX_LEARNERS
    calls, twins = _learners(pkg, env3, RAGGED[0], "global", K, seed=3)
    got = SweepCall(pkg, env3, calls).step()  # (two select launches: learners 8 .. 15 come from the second)
    for k, twin in enumerate(twins):
        same_bits(got[k], twin.step(), f"learner {k}")


def test_n_zero_zeroes_the_losses_and_changes_nothing_else(pkg, env3):
    def edit(k, batch):
        for key in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "idx"):
            batch[key] = batch[key][:0]

    calls, _ = _learners(pkg, env3, RAGGED[1], "perspective", 3, seed=4, edit=edit)
    before = [[flat(m) for m in c.models] for c in calls]
    got = SweepCall(pkg, env3, calls).step()
    for k in range(3):
        assert np.array_equal(got[k][0], [0.0, 0.0])
        for t in range(2):
            assert got[k][1][t]["step"] == 0.0 and np.array_equal(got[k][1][t]["params"], before[k][t].astype(np.float32).astype(np.float64))
            assert not got[k][1][t]["exp_avg"].any() and not got[k][1][t]["exp_avg_sq"].any()


# ---- 4. the dropout form -----------------------------------------------------------------------------------------------------------------------
DROP_CASE = (33, 2, 2, ([4], 3, [1], [1], [1], 3, 33, [6]), ([4], 3, [1], [1], [1], 3, 33, [6]))  # rnn layers 3, hidden 33, T 2


def test_dropout_sweep_is_bitwise_the_dropout_step(pkg, env3):
    calls, twins = _learners(pkg, env3, DROP_CASE, "global", 2, seed=5)
    for c in calls + twins:
        dropout_workspace(pkg, env3, c)
    drops = [make_drop(pkg, 0.2, 0.2, seed=11, offset=3), make_drop(pkg, 0.5, 0.0, seed=(1 << 40) + 7, offset=(1 << 33) + 1)]
    got = SweepCall(pkg, env3, calls, drops).step()
    for k, twin in enumerate(twins):
        same_bits(got[k], dropout_step(pkg, env3, twin, drops[k]), f"learner {k}")
    # the masks matter: the plain step on a third copy gives other bytes
    plain = _learners(pkg, env3, DROP_CASE, "global", 2, seed=5)[0][0].step()
    assert not np.array_equal(plain[1][0]["bits"][0], got[0][1][0]["bits"][0])


def test_dropout_sweep_with_every_p_zero_is_the_plain_sweep(pkg, env3):
    calls, twins = _learners(pkg, env3, DROP_CASE, "perspective", 2, seed=6)
    for c in calls:
        dropout_workspace(pkg, env3, c)
    got = SweepCall(pkg, env3, calls, [make_drop(pkg, 0.0, 0.0, seed=1, offset=0), make_drop(pkg, 0.0, 0.0, seed=2, offset=5)]).step()
    want = SweepCall(pkg, env3, twins).step()
    for k in range(2):
        same_bits(got[k], want[k], f"learner {k}")


# ---- 5. graph replay ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(pkg, env3):
    calls, twins = _learners(pkg, env3, RAGGED[1], "global", 2, seed=7)
    want = [[twin.step() for twin in twins] for _ in range(3)]
    sweep = SweepCall(pkg, env3, calls)
    sweep.step()  # one eager step first: the recurrence kernels' LDS ceilings (step 1 of 3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    state = [g[key].buf for c in calls for g in c.bufs for key in ("params", "exp_avg", "exp_avg_sq")] + [g["step"] for c in calls for g in c.bufs]
    saved = [x.clone() for x in state]
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            sweep.launch()
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip(state, saved):  # (capturing runs nothing; restore in case the runtime did)
        x.copy_(sv)
    for step in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        got = sweep.results()
        for k in range(2):
            same_bits(got[k], want[step][k], f"replay {step} learner {k}")


# ---- 6. refusals leave memory untouched --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_parameters_untouched(pkg, env3):
    L = pkg._lib
    calls, _ = _learners(pkg, env3, RAGGED[1], "global", 3, seed=8)
    other = _learners(pkg, env3, RAGGED[2], "global", 1, seed=8)[0][0]  # another shape (T 8, other networks)
    state = lambda cs: [g[key].buf.clone() for c in cs for g in c.bufs for key in ("params", "exp_avg", "exp_avg_sq")]
    everyone = calls + [other]
    before = state(everyone)

    def refused(sweep, *words):
        with torch.cuda.device(DEV):
            assert sweep.call() == L.E_INVALID
        msg = env3.lib.susnet_last_error().decode()
        assert msg.startswith("susnet_spatial_train_sweep: ") and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(state(everyone), before)), "a refused call wrote"

    refused(SweepCall(pkg, env3, [calls[0], calls[1], other]), "learner 2: ", "differs from learner 0's")
    shared = SweepCall(pkg, env3, calls)
    shared.ios[2].team[1].params = shared.ios[0].team[0].params
    refused(shared, "learner 2: team[1].params is shared with learner 0")
    got = SweepCall(pkg, env3, calls).step()  # the same learners are served as they are
    assert all(got[k][1][t]["step"] == 3.0 for k in range(3) for t in range(2))


# ---- 7. the trainer takes the path -------------------------------------------------------------------------------------------------------------
def _members(pkg, K, Fz, batch=8, T=2, hidden=None, dropout_seed=None, dropout=0.0):
    """K spatial trainers on real 1v2 envs with rings, built twice from the same seeds (the sweep's members and their twins)."""
    out = []
    for _ in range(2):
        members = []
        for k in range(K):
            env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device=DEV, rng="philox", seed=40 + k, auto_reset=True, grid_size=14,
                                         shuffle_imposter_index=True)
            fz = Fz(env)
            _, planes, non = env._make_obs(fz.config, 1, rows=1)
            Fn = non.shape[-1] + (env.n_agents if Fz is pkg.GlobalFeaturizer else 0)
            H = (hidden or {}).get(k, 16)
            mk = lambda n_actions, seed: make_model(pkg, planes.shape[-1], planes.shape[-3], Fn, [4], [1], [1], 3, [1], 2, H, [12], n_actions, seed,
                                                    dropout=dropout)
            imp, crew = mk(env.n_imposter_actions, 10 * k + 1), mk(env.n_crew_actions, 10 * k + 2)
            tr = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], LRS[k % 3], GAMMAS[k % 3], featurizer=fz, spatial=True,
                                          rnn_dropout_seed=None if dropout_seed is None else dropout_seed + k)
            ring = pkg.DeviceReplayBuffer(env.batch * 6, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
            ring.populate_fused(env, 6)
            members.append((tr, ring))
        out.append(members)
    return out


def _same_trainers(a, b, what):
    for t in range(2):
        assert torch.equal(a.flat[t], b.flat[t]), f"{what} team {t} parameters"
        for x, y in zip(a.state_tensors(t), b.state_tensors(t)):
            assert torch.equal(x, y), f"{what} team {t} Adam state"


@pytest.mark.parametrize("dropout_seed", [None, 5])
@pytest.mark.parametrize("Fz", ["GlobalFeaturizer", "PerspectiveFeaturizer"])
def test_sweep_trainer_takes_the_path_and_matches_the_members_own_steps(pkg, Fz, dropout_seed):
    Fz = getattr(pkg, Fz)
    kw = dict(dropout_seed=dropout_seed, dropout=0.0 if dropout_seed is None else 0.2)
    members, twins = _members(pkg, 3, Fz, **kw)
    sweep = pkg.DeviceDQNSweepTrainer([m[0] for m in members])
    rings = [m[1] for m in members]
    assert sweep.compatible() and sweep.uses_spatial(rings) and not sweep.uses_hip(rings)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    for step in range(2):
        idxs = [torch.randint(0, r.size, (24,), device=DEV, generator=g) for r in rings]
        out = sweep.train_step_on_indices(rings, idxs)
        for k, (tr, ring) in enumerate(twins):
            assert torch.equal(out[k], tr.train_step_on_indices(ring, idxs[k])), f"step {step} member {k} losses"
            _same_trainers(members[k][0], tr, f"step {step} member {k}")
            assert members[k][0].dropout_steps == tr.dropout_steps == (0 if dropout_seed is None else step + 1)
    assert float(members[0][0].step_count[1]) > 0
    # one member of another hidden width: the per-member loop, and still every member's own step
    members, twins = _members(pkg, 3, Fz, hidden={1: 12}, **kw)
    sweep = pkg.DeviceDQNSweepTrainer([m[0] for m in members])
    rings = [m[1] for m in members]
    assert not sweep.compatible() and not sweep.uses_spatial(rings)
    idxs = [torch.randint(0, r.size, (24,), device=DEV, generator=g) for r in rings]
    out = sweep.train_step_on_indices(rings, idxs)
    for k, (tr, ring) in enumerate(twins):
        assert torch.equal(out[k], tr.train_step_on_indices(ring, idxs[k]))
        _same_trainers(members[k][0], tr, f"fallback member {k}")


def test_more_members_than_one_call_carries(pkg):
    K = pkg._lib.SPATIAL_SWEEP_MAX_LEARNERS + 1
    assert pkg.trainer.sweep_chunks(K, pkg._lib.SPATIAL_SWEEP_MAX_LEARNERS) == [(0, K - 1), (K - 1, K)]
    members, twins = _members(pkg, K, pkg.GlobalFeaturizer, batch=4, T=1)
    sweep = pkg.DeviceDQNSweepTrainer([m[0] for m in members])
    rings = [m[1] for m in members]
    assert sweep.uses_spatial(rings)
    idxs = [torch.arange(3, device=DEV) + k for k in range(K)]
    out = sweep.train_step_on_indices(rings, idxs)
    for k, (tr, ring) in enumerate(twins):
        assert torch.equal(out[k], tr.train_step_on_indices(ring, idxs[k])), k
        _same_trainers(members[k][0], tr, f"member {k}")


# ---- 8. the loop ---------------------------------------------------------------------------------------------------------------------------------
def _raw_env(pkg, seed, batch=8):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                  obs=pkg.ObsConfig("raw", dtype=torch.uint8), max_time_steps=6)


def _spatial_models(pkg, env, seed):
    _, planes, non = env._make_obs(pkg.ObsConfig("planes"), 1, rows=1)
    cfg = dict(strides=[1], paddings=[1], kernel_size=[3, 3], dilations=[1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[12],
               input_image_size=planes.shape[-1], non_spatial_input_size=non.shape[-1] + env.n_agents, n_channels=[planes.shape[-3], 6])
    out = []
    for s, n in ((seed, env.n_imposter_actions), (seed + 1, env.n_crew_actions)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(s)
            out.append(pkg.SpatialDQN(**cfg, n_actions=n).to(DEV))
    return out


def _loop_member(pkg, k, save_dir, T=2):
    env = _raw_env(pkg, 70 + k)
    imp, crew = _spatial_models(pkg, env, 10 * k + 3)
    fz = pkg.GlobalFeaturizer(env)
    policy = pkg.WindowedPolicyRollout(env, fz, imp, crew, sequence_length=T, mask_dead=True, kernels=True)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], lr=LRS[k], gamma=GAMMAS[k], policy=policy, featurizer=fz, spatial=True)
    ring = pkg.DeviceReplayBuffer(env.batch * 9, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 3)
    g = torch.Generator(device=DEV)
    g.manual_seed(k)
    return (env, pkg.EpisodicMetricHandler(), ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.05, 100), save_dir, g)


def test_train_sweep_matches_separate_train_runs(pkg, tmp_path):
    kw = dict(train_step_interval=5, batch_size=4, num_saves=5, target_update_interval=10)
    members = [_loop_member(pkg, k, tmp_path / f"sweep{k}") for k in range(3)]
    sweep = pkg.DeviceDQNSweepTrainer([m[4] for m in members])
    assert sweep.uses_spatial([m[2] for m in members])
    logs = pkg.train_sweep(members, 20, **kw)
    for k in range(3):
        env, metrics, ring, policy, trainer, sched, save_dir, gen = _loop_member(pkg, k, tmp_path / f"alone{k}")
        log = pkg.train(env, metrics, 20, ring, policy, trainer, sched, save_dir, generator=gen, **kw)
        m = members[k]
        _same_trainers(m[4], trainer, f"member {k}")
        assert float(trainer.step_count[0]) > 0
        for name in (pkg.SusMetrics.IMPOSTER_LOSS, pkg.SusMetrics.CREW_LOSS, pkg.SusMetrics.AVG_IMPOSTER_RETURNS, pkg.SusMetrics.AVG_CREW_RETURNS):
            assert m[1].metrics[name] == metrics.metrics[name], name
        assert len(metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS]) == 4  # train ticks 0, 5, 10, 15
        ra, rb = logs[k].records(), log.records()
        assert ra.keys() == rb.keys() and ra["count"] == rb["count"] > 0
        for key in ra:
            np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
        names = sorted(p.name for p in (tmp_path / f"sweep{k}").iterdir())
        assert names == sorted(p.name for p in (tmp_path / f"alone{k}").iterdir()) and "imposter_spatial_dqn_100%.pt" in names
        for name in names:
            a = torch.load(tmp_path / f"sweep{k}" / name, map_location="cpu", weights_only=False)
            b = torch.load(tmp_path / f"alone{k}" / name, map_location="cpu", weights_only=False)
            sa, sb = a.get("state_dict", a), b.get("state_dict", b)
            assert sa.keys() == sb.keys() and all(torch.equal(sa[key], sb[key]) for key in sa if torch.is_tensor(sa[key])), name


def test_run_sweep_writes_one_experiment_directory_per_variant(pkg, tmp_path):
    common = dict(num_steps=11, imposter_model_factory=lambda env: _spatial_models(pkg, env, 1)[0],
                  crew_model_factory=lambda env: _spatial_models(pkg, env, 1)[1], components=[], sequence_length=2, replay_buffer_size=8 * 16,
                  replay_prepopulate_steps=3, batch_size=4, scheduler_time_steps=100, experiment_base_dir=tmp_path,
                  featurizer_factory=lambda env: pkg.GlobalFeaturizer(env))
    handlers = pkg.run_sweep(lambda seed: _raw_env(pkg, seed), [{"gamma": 0.9, "name": "g0.9", "seed": 1}, {"gamma": 0.8, "seed": 2}], **common)
    assert len(handlers) == 2 and sorted(p.name for p in tmp_path.iterdir()) == ["1", "g0.9"]
    for name, gamma, handler in (("g0.9", 0.9, handlers[0]), ("1", 0.8, handlers[1])):
        (stamp,) = list((tmp_path / name).iterdir())
        config = json.loads((stamp / "config.json").read_text())
        assert config["gamma"] == gamma and config["train_step"] == "susnet_spatial_train_sweep" and config["featurizer_type"] == "global"
        assert config["imposter_model_type"] == "spatial_dqn" and config["sequence_length"] == 2
        saved = json.loads((stamp / "metrics.json").read_text())
        assert len(saved["imposter_loss"]) == 3 and len(handler.metrics[pkg.SusMetrics.AVG_IMPOSTER_RETURNS]) > 0
        assert (stamp / "imposter_spatial_dqn_100%.pt").exists() and (stamp / "crew_spatial_dqn_0.pt").exists()
