"""The dense learner's sweep step (susnet_mlp_train_sweep; DeviceDQNSweepTrainer over dense=True trainers; run_sweep(dense_train=True)) on
the MI355X.  The oracle throughout is the single-learner step, susnet_mlp_train_step, which test_gpu_mlp_train.py and
test_gpu_train_exact.py pin to float64 and exact references: every comparison here is bit for bit, a learner of the sweep against its
twin -- built from the same seeds -- taking its own steps."""
import importlib
import json

import numpy as np
import pytest
import torch

from mlp_sweep_util import GAMMAS, LRS, Learner, assert_same, build, documented_grid, make_batch, make_teams, sweep_call, sweep_step
from train_exact import DEV

pytestmark = pytest.mark.gpu

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
RAGGED_STACKS = [[27, 12, 9, 8, 8, 9, 10, 5], [131, 33, 31, 5], [19, 7]]  # test_gpu_mlp_train.py's


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env4(pkg):
    """A 4-agent, one-imposter handle: the call takes the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


def _crew(dims):
    return dims[:-1] + [dims[-1] + 2]


def _check(members, twins, what):
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(members, twins)):
        assert_same(a, b, f"{what} learner {k}")
        a.check_canaries()
        b.check_canaries()


# ---- 1. bitwise the single step, two consecutive steps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("dims", RAGGED_STACKS, ids=["7layers", "131-33-31-5", "19-7"])
def test_sweep_is_bitwise_the_single_step(pkg, env4, dims, n):
    members, twins = build(pkg, env4, 3, (dims, _crew(dims)), n, seed=n)
    before = [m.snapshot() for m in members]
    for step in range(2):
        sweep_step(pkg, members)
        for t in twins:
            t.step()
        _check(members, twins, f"step {step}")
    # the learners are three different ones, and every one of them moved
    for j, k in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(members[j].bufs[0]["params"].view, members[k].bufs[0]["params"].view)
    for m, b in zip(members, before):
        assert any(not torch.equal(x, y) for (_, x), y in zip(m.written(), b))
        assert sum(m.steps()) >= 2 * 4  # per call: four agents' crew updates at least, and the imposter's


# ---- 2. a workgroup walking more than one tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n", [([131, 33, 31, 5], 8225), ([1024, 256, 256, 32], 1601)], ids=["grid-cap", "partial-cap"])
def test_a_workgroup_walks_more_than_one_tile(pkg, env4, dims, n):
    """8 225 rows are 258 tiles against at most 256 workgroups, the last tile one row; [1024, 256, 256, 32] has Pp = 336 420, so the 64 MiB
    of partials allow 49 workgroups against 51 tiles.  Agent 3 is never the imposter: its crew list holds all n rows."""
    G, tiles = documented_grid((dims, dims), n)
    assert tiles > G, (tiles, G)
    assert (G, tiles) == ((256, 258) if n == 8225 else (49, 51))
    members, twins = build(pkg, env4, 2, (dims, dims), n, seed=2, imposter_agents=[0, 1, 2])
    for m in members:
        assert not bool((m.tensors["imposters"][m.tensors["idx"]] == 3).any())  # the (agent 3, crew) list: n rows, more tiles than workgroups
    sweep_step(pkg, members)
    for t in twins:
        t.step()
    _check(members, twins, "one step")
    assert members[0].steps() == twins[0].steps() and members[0].steps()[1] == 4.0


# ---- 3. ragged learners -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crew", [True, False], ids=["both-teams", "imposters-only"])
def test_ragged_learners(pkg, env4, crew):
    """Learner 0 has no imposter rows for agent 0 (an empty list: no step for that update, whatever the others do), learner 1 only done
    rows, learner 2 is ordinary."""
    dims = [131, 33, 31, 5]
    members, twins = build(pkg, env4, 3, (dims, _crew(dims) if crew else None), 33, seed=3, M=200,
                           per_learner={0: dict(imposter_agents=[1, 2, 3]), 1: dict(all_done=True)})
    for step in range(2):
        sweep_step(pkg, members)
        for t in twins:
            t.step()
        _check(members, twins, f"step {step}")
    drawn = [set(m.tensors["imposters"][m.tensors["idx"]].reshape(-1).tolist()) for m in members]
    assert 0 not in drawn[0] and drawn[2] == {0, 1, 2, 3}
    assert [m.steps()[0] for m in members] == [2.0 * len(d) for d in drawn]  # one imposter step per agent that has rows, per call
    assert members[0].steps()[0] < members[2].steps()[0]


def test_an_empty_batch_zeroes_the_losses_and_nothing_else(pkg, env4):
    dims = [19, 7]
    rng = np.random.default_rng(5)
    members = []
    for k in range(3):
        batch = make_batch(rng, dims[0], dims[-1], 0, M=9)
        members.append(Learner(pkg, env4, make_teams(rng, (dims, _crew(dims)), LRS[k]), batch, GAMMAS[k], losses_fill=7.0))
    before = [m.snapshot() for m in members]
    sweep_step(pkg, members)
    torch.cuda.synchronize()
    for m, b in zip(members, before):
        m.check_canaries()
        assert m.losses[1:3].tolist() == [0.0, 0.0]
        for ((name, x), y) in list(zip(m.written(), b))[1:]:
            assert torch.equal(x, y), name


# ---- 4. chunk edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 16])
def test_one_learner_and_a_full_table(pkg, env4, K):
    assert pkg._lib.MLP_SWEEP_MAX_LEARNERS == 16
    members, twins = build(pkg, env4, K, ([19, 7], [19, 9]), 33, seed=4)
    sweep_step(pkg, members)
    for t in twins:
        t.step()
    _check(members, twins, f"K = {K}")
    assert all(sum(m.steps()) > 0 for m in members)
    if K == 16:  # one learner more is refused before anything is launched
        extra = build(pkg, env4, 1, ([19, 7], [19, 9]), 33, seed=44, twins=1)[0]
        assert sweep_call(pkg, members + extra) == pkg._lib.E_INVALID and b"n_learners" in env4.lib.susnet_last_error()
        _check(members, twins, "after the refusal")


# ---- 5. reproducible and capturable -----------------------------------------------------------------------------------------------------------
def test_two_runs_from_equal_state_leave_equal_bytes(pkg, env4):
    a, b = build(pkg, env4, 3, ([131, 33, 31, 5], [131, 33, 31, 7]), 65, seed=6)
    for step in range(2):
        sweep_step(pkg, a)
        sweep_step(pkg, b)
        _check(a, b, f"step {step}")


def test_graph_replay_matches_eager(pkg, env4):
    """One eager call (it sets the gradient kernel's LDS ceiling), a capture of one call, two replays: three eager calls of the twins."""
    members, twins = build(pkg, env4, 3, ([131, 33, 31, 5], [131, 33, 31, 7]), 65, seed=7)
    sweep_step(pkg, members)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            sweep_step(pkg, members)
    torch.cuda.current_stream().wait_stream(s)
    for t in twins:
        t.step()
    _check(members, twins, "the capture itself runs nothing: one step")
    for k in range(2):
        graph.replay()
        for t in twins:
            t.step()
        _check(members, twins, f"replay {k}")


# ---- 6. the trainer takes the path ------------------------------------------------------------------------------------------------------------
def _flat_env(pkg, seed, batch=64, **kw):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9, shuffle_imposter_index=True,
                                  obs=pkg.ObsConfig("flat", COMPS3), **kw)


def _mlp(pkg, dims, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return pkg.MLP(dims).to(DEV)


def _window_models(pkg, env, T, seed, hidden=(48, 24)):
    F = env.obs.shape[-1]
    return _mlp(pkg, [T * F, *hidden, env.n_imposter_actions], seed), _mlp(pkg, [T * F, *hidden, env.n_crew_actions], seed + 1)


def _members(pkg, K, T, hidden=None):
    """K dense trainers on real base 1v3 9x9 envs with rings of 384 rows, built twice from the same seeds."""
    out = []
    for _ in range(2):
        members = []
        for k in range(K):
            env = _flat_env(pkg, 40 + k)
            imp, crew = _window_models(pkg, env, T, 10 * k + 1, **({"hidden": hidden[k]} if hidden and k in hidden else {}))
            tr = pkg.DeviceDQNTeamTrainer(env, imp, crew, COMPS3, LRS[k % 3], GAMMAS[k % 3], dense=True, sequence_length=T)
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


@pytest.mark.parametrize("T", [1, 2])
def test_sweep_trainer_takes_the_path_and_matches_the_members_own_steps(pkg, T):
    members, twins = _members(pkg, 3, T)
    sweep = pkg.DeviceDQNSweepTrainer([m[0] for m in members])
    rings = [m[1] for m in members]
    assert sweep.compatible() and sweep.uses_dense(rings) and not sweep.uses_hip(rings) and not sweep.uses_spatial(rings)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    for step in range(2):
        idxs = [torch.randint(0, r.size, (40,), device=DEV, generator=g) for r in rings]
        out = sweep.train_step_on_indices(rings, idxs)
        for k, (tr, ring) in enumerate(twins):
            assert torch.equal(out[k], tr.train_step_on_indices(ring, idxs[k])), f"step {step} member {k} losses"
            _same_trainers(members[k][0], tr, f"step {step} member {k}")
    assert float(members[0][0].step_count[1]) > 0 and bool((out > 0).all())
    # one member of another stack: the per-member loop, and still every member's own step
    members, twins = _members(pkg, 3, T, hidden={1: (40, 24)})
    sweep = pkg.DeviceDQNSweepTrainer([m[0] for m in members])
    rings = [m[1] for m in members]
    assert all(tr.uses_dense(r) for tr, r in members) and not sweep.compatible() and not sweep.uses_dense(rings)
    idxs = [torch.randint(0, r.size, (40,), device=DEV, generator=g) for r in rings]
    out = sweep.train_step_on_indices(rings, idxs)
    for k, (tr, ring) in enumerate(twins):
        assert torch.equal(out[k], tr.train_step_on_indices(ring, idxs[k]))
        _same_trainers(members[k][0], tr, f"fallback member {k}")


# ---- 7. the loop --------------------------------------------------------------------------------------------------------------------------------
VARIANTS = [{"gamma": 0.99, "name": "g0.99", "seed": 1}, {"gamma": 0.9, "name": "g0.9", "seed": 2}, {"gamma": 0.8, "learning_rate": 3e-4, "seed": 3}]
LOOP = dict(num_steps=12, sequence_length=2, replay_buffer_size=8 * 16, replay_prepopulate_steps=3, batch_size=8, scheduler_time_steps=100,
            train_step_interval=4, num_checkpoint_saves=2, target_update_interval=8, learning_rate=1e-3)


def _loop_env(pkg, seed):
    return _flat_env(pkg, seed, batch=8, max_time_steps=6)


def test_run_sweep_runs_the_reference_window_on_the_dense_sweep(pkg, tmp_path):
    T = LOOP["sequence_length"]
    handlers = pkg.run_sweep(lambda seed: _loop_env(pkg, seed), VARIANTS, imposter_model_factory=lambda env: _window_models(pkg, env, T, 5)[0],
                             crew_model_factory=lambda env: _window_models(pkg, env, T, 5)[1], components=COMPS3, dense_train=True,
                             experiment_base_dir=tmp_path / "sweep", **LOOP)
    assert len(handlers) == 3 and sorted(p.name for p in (tmp_path / "sweep").iterdir()) == ["2", "g0.9", "g0.99"]
    for k, (variant, handler) in enumerate(zip(VARIANTS, handlers)):
        (stamp,) = list((tmp_path / "sweep" / str(variant.get("name", k))).iterdir())
        config = json.loads((stamp / "config.json").read_text())
        assert config["sequence_length"] == 2 and config["train_step"] == "susnet_mlp_train_sweep" and config["gamma"] == variant["gamma"]
        assert config["seed"] == variant["seed"] and list(config)[-2:] == ["seed", "train_step"]
        # the twin member, as run_experiment builds its run, through train() alone
        seed = variant["seed"]
        env = _loop_env(pkg, seed)
        imp, crew = _window_models(pkg, env, T, 5)
        policy = pkg.PolicyRollout(env, imp, crew, components=COMPS3, mask_dead=True, dense=True, sequence_length=T)
        trainer = pkg.DeviceDQNTeamTrainer(env, imp, crew, COMPS3, lr=variant.get("learning_rate", LOOP["learning_rate"]), gamma=variant["gamma"],
                                           policy=policy, dense=True, sequence_length=T)
        ring = pkg.DeviceReplayBuffer(LOOP["replay_buffer_size"], env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
        assert trainer.uses_dense(ring)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        ring.populate_fused(env, LOOP["replay_prepopulate_steps"])
        metrics = pkg.EpisodicMetricHandler()
        alone = tmp_path / f"alone{k}"
        pkg.train(env, metrics, LOOP["num_steps"], ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.05, LOOP["scheduler_time_steps"]), alone,
                  train_step_interval=LOOP["train_step_interval"], batch_size=LOOP["batch_size"], num_saves=LOOP["num_checkpoint_saves"],
                  target_update_interval=LOOP["target_update_interval"], generator=gen, per_episode_info=True)
        for name in (pkg.SusMetrics.IMPOSTER_LOSS, pkg.SusMetrics.CREW_LOSS):
            assert handler.metrics[name] == metrics.metrics[name] and len(metrics.metrics[name]) == 3 and all(v > 0 for v in metrics.metrics[name]), name
        names = sorted(p.name for p in alone.iterdir())
        assert names and all((stamp / name).exists() for name in names)
        for name in names:
            a = torch.load(stamp / name, map_location="cpu", weights_only=False)
            b = torch.load(alone / name, map_location="cpu", weights_only=False)
            sa, sb = a.get("state_dict", a), b.get("state_dict", b)
            assert sa.keys() == sb.keys() and all(torch.equal(sa[key], sb[key]) for key in sa if torch.is_tensor(sa[key])), name


def test_a_compiled_in_layout_keeps_the_fused_sweep(pkg, tmp_path):
    """dense_train=True at T = 1 on a layout susnet_dqn_train_sweep serves: built and swept as before, config.json without `train_step`."""
    def env_factory(seed):
        return pkg.BatchedFourRoomEnv(1, 2, 4, batch=8, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=14, shuffle_imposter_index=True,
                                      obs=pkg.ObsConfig("flat", COMPS3), max_time_steps=6)
    seen = []
    real = pkg.DeviceDQNSweepTrainer.train_step_on_indices

    def spy(self, rings, idxs):
        seen.append((self.uses_hip(rings), self.uses_dense(rings)))
        return real(self, rings, idxs)

    pkg.DeviceDQNSweepTrainer.train_step_on_indices = spy
    try:
        pkg.run_sweep(env_factory, VARIANTS[:2], imposter_model_factory=lambda env: pkg.policy.reference_imposter_mlp(env, COMPS3, seed=3),
                      crew_model_factory=lambda env: pkg.policy.reference_crew_mlp(env, COMPS3, seed=4), components=COMPS3, dense_train=True,
                      experiment_base_dir=tmp_path, **dict(LOOP, sequence_length=1))
    finally:
        pkg.DeviceDQNSweepTrainer.train_step_on_indices = real
    assert seen and all(s == (True, False) for s in seen)
    for name in ("g0.99", "g0.9"):
        (stamp,) = list((tmp_path / name).iterdir())
        config = json.loads((stamp / "config.json").read_text())
        assert "train_step" not in config and config["sequence_length"] == 1 and list(config)[-1] == "seed"
