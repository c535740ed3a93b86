"""The sweep train step (susnet_dqn_train_sweep, DeviceDQNSweepTrainer, train_sweep, run_sweep) on the MI355X: every member's result is
BITWISE what its own single-learner step (susnet_dqn_train_step, DeviceDQNTeamTrainer) leaves -- the contract that makes a sweep a
drop-in for the reference's loop over run_experiment(**config) (notebooks/experiment_1v1.ipynb, experiment_mlp.ipynb)."""
import copy
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
GAMMAS, LRS = (0.99, 0.9, 0.8), (1e-3, 3e-4, 1e-4)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _env_1v2(pkg, seed, batch=128):
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=14,
                                  shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3))


def _env_1v1(pkg, seed, comps, batch=64, walls=False):
    kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
    return pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, walls), batch=batch, device="cuda:0", rng="philox", seed=seed,
                                             auto_reset=True, obs=pkg.ObsConfig("flat", comps))


def _ring(pkg, env, ticks=4):
    ring = pkg.DeviceReplayBuffer(env.batch * ticks, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, ticks)
    return ring


class Member:
    """One learner and its twin: same env, ring and initial weights; the twin steps alone (susnet_dqn_train_step)."""

    def __init__(self, pkg, env, comps, k, crew, gamma, lr):
        self.env, self.ring = env, _ring(pkg, env)
        imp = pkg.policy.reference_imposter_mlp(env, comps, seed=10 + k)
        cr = pkg.policy.reference_crew_mlp(env, comps, seed=40 + k) if crew else None
        imp2, cr2 = copy.deepcopy(imp), copy.deepcopy(cr)
        self.policy = pkg.PolicyRollout(env, imp, cr, comps)
        self.twin_policy = pkg.PolicyRollout(env, imp2, cr2, comps)
        self.trainer = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, lr, gamma, train_crew=crew, policy=self.policy)
        self.twin = pkg.DeviceDQNTeamTrainer(env, imp2, cr2, comps, lr, gamma, train_crew=crew, policy=self.twin_policy)


def _members_1v2(pkg, K=3):
    return [Member(pkg, _env_1v2(pkg, seed=20 + k), COMPS3, k, True, GAMMAS[k % 3], LRS[k % 3]) for k in range(K)]


def _assert_same(members, losses=None, twin_losses=None):
    for k, m in enumerate(members):
        a, b = m.trainer, m.twin
        for t in range(2):
            if not a.trained[t]:
                continue
            for name in ("flat", "exp_avg", "exp_avg_sq", "step_count"):
                assert torch.equal(getattr(a, name)[t], getattr(b, name)[t]), (k, t, name)
        for net, twin_net in ((m.policy.fused_imposter, m.twin_policy.fused_imposter), (m.policy.fused_crew, m.twin_policy.fused_crew)):
            if net is not None:
                assert torch.equal(net.packed, twin_net.packed), k
    if losses is not None:
        assert torch.equal(losses, twin_losses)


def _step_both(sweep, members, idxs):
    rings = [m.ring for m in members]
    losses = sweep.train_step_on_indices(rings, idxs)
    twin_losses = torch.stack([m.twin.train_step_on_indices(m.ring, i) for m, i in zip(members, idxs)])
    return losses, twin_losses


def _draw(members, n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return [torch.randint(0, m.ring.size, (n,), device="cuda:0", generator=g) for m in members]


def test_sweep_is_bitwise_the_single_learner_step_1v2(pkg):
    """K = 3 on 1v2, dims [88,256,128,64,16,7] / [..,6], both teams, gamma 0.99 / 0.9 / 0.8, lr 1e-3 / 3e-4 / 1e-4, N = 40: one full tile
    and a ragged tile of 8 (two workgroups per learner); three consecutive steps."""
    members = _members_1v2(pkg)
    assert members[0].trainer._dims[0] == [88, 256, 128, 64, 16, 7]
    sweep = pkg.DeviceDQNSweepTrainer([m.trainer for m in members])
    assert sweep.uses_hip([m.ring for m in members])
    for s in range(3):
        losses, twin_losses = _step_both(sweep, members, _draw(members, 40, s))
        assert losses.shape == (3, 2) and bool((losses > 0).all())
        _assert_same(members, losses, twin_losses)
    assert all(float(m.trainer.step_count[t]) > 0 for m in members for t in range(2))
    assert not torch.equal(members[0].trainer.flat[0], members[1].trainer.flat[0])


def test_ragged_learners_skip_their_empty_updates(pkg):
    """N = 8; member 1 samples no row whose imposter is agent 1, member 2 only rows whose imposter is agent 0: their empty (agent, team)
    lists take no step and do not advance the step count (train.py:101), whatever the other learners of the launch do."""
    members = _members_1v2(pkg)
    idxs = []
    for k, m in enumerate(members):
        imp = m.ring.imposters[:m.ring.size, 0].cpu().numpy()
        rows = np.arange(len(imp)) if k == 0 else np.flatnonzero(imp != 1) if k == 1 else np.flatnonzero(imp == 0)
        assert len(rows) >= 8
        idxs.append(torch.tensor(rows[:8], device="cuda:0"))
    imp1 = members[1].ring.imposters[idxs[1], 0]
    imp2 = members[2].ring.imposters[idxs[2], 0]
    assert int((imp1 == 1).sum()) == 0  # member 1: the imposter list of agent 1 is empty
    assert int((imp2 != 0).sum()) == 0  # member 2: the imposter lists of agents 1 and 2 and the crew list of agent 0 are empty
    assert len(set(members[0].ring.imposters[idxs[0], 0].tolist())) > 1
    sweep = pkg.DeviceDQNSweepTrainer([m.trainer for m in members])
    losses, twin_losses = _step_both(sweep, members, idxs)
    _assert_same(members, losses, twin_losses)
    # 3 agents x 2 teams = 6 possible updates, 3 per team; member 2's imposter team steps once (agent 0), its crew team twice (agents 1, 2)
    assert float(members[2].trainer.step_count[0]) == 1.0 and float(members[2].trainer.step_count[1]) == 2.0
    assert float(members[1].trainer.step_count[0]) <= 2.0
    for m in members:
        for t in range(2):
            assert float(m.trainer.step_count[t]) == float(m.twin.step_count[t])


def test_sixteen_learners_smallest_batch_and_incompatible_fallback(pkg):
    """The notebooks' shape -- 1v1, onehot_pos, imposter only -- at K = 16 (SUSNET_DQN_MAX_LEARNERS), N = 8, two steps.  Then one member on
    the wall map: the library refuses the mix (the grids differ), the sweep trainer runs the members' own steps instead, same result."""
    comps = ["onehot_pos"]
    members = [Member(pkg, _env_1v1(pkg, 30 + k, comps), comps, k, False, GAMMAS[k % 3], LRS[k % 3]) for k in range(16)]
    sweep = pkg.DeviceDQNSweepTrainer([m.trainer for m in members])
    assert sweep.uses_hip([m.ring for m in members])
    for s in range(2):
        losses, twin_losses = _step_both(sweep, members, _draw(members, 8, 100 + s))
        assert losses.shape == (16, 2)
        _assert_same(members, losses, twin_losses)
    assert all(float(m.trainer.step_count[0]) == 2.0 for m in members)
    # a member on another grid
    mixed = members[:3] + [Member(pkg, _env_1v1(pkg, 77, comps, walls=True), comps, 3, False, 0.9, 1e-3)]
    sweep2 = pkg.DeviceDQNSweepTrainer([m.trainer for m in mixed])
    rings = [m.ring for m in mixed]
    assert all(m.trainer.uses_hip(m.ring) for m in mixed) and not sweep2.compatible() and not sweep2.uses_hip(rings)
    idxs = _draw(mixed, 8, 7)
    L = pkg._lib
    ios, envs = (L.DqnIO * 4)(), (C.c_void_p * 4)()
    for k, m in enumerate(mixed):
        ios[k], envs[k] = m.trainer._hip_io(m.ring, idxs[k]), m.env._h
    before = [m.trainer.flat[0].clone() for m in mixed]
    assert mixed[0].env.lib.susnet_dqn_train_sweep(envs, ios, 4, mixed[0].env._stream()) == L.E_INVALID
    msg = mixed[0].env.lib.susnet_last_error()
    assert b"learner 3" in msg and b"grid" in msg
    torch.cuda.synchronize()
    assert all(torch.equal(b, m.trainer.flat[0]) for b, m in zip(before, mixed))
    losses, twin_losses = _step_both(sweep2, mixed, idxs)
    _assert_same(mixed, losses, twin_losses)
    assert float(mixed[3].trainer.step_count[0]) == 1.0


def test_coordinate_layout(pkg):
    """1v1 coord_pos (the third compiled-in row type), K = 2, N = 33: two workgroups per learner, the second with one row."""
    comps = ["coord_pos"]
    members = [Member(pkg, _env_1v1(pkg, 50 + k, comps), comps, k, False, GAMMAS[k], LRS[k]) for k in range(2)]
    sweep = pkg.DeviceDQNSweepTrainer([m.trainer for m in members])
    assert sweep.uses_hip([m.ring for m in members])
    for s in range(2):
        losses, twin_losses = _step_both(sweep, members, _draw(members, 33, 200 + s))
        _assert_same(members, losses, twin_losses)


def test_graph_replay_matches_eager(pkg):
    """One captured sweep step (K = 3, 1v2, N = 32) replayed twice after an eager step = three eager steps of a twin sweep."""
    members = _members_1v2(pkg)
    twins = pkg.DeviceDQNSweepTrainer([m.twin for m in members])
    sweep = pkg.DeviceDQNSweepTrainer([m.trainer for m in members])
    rings = [m.ring for m in members]
    idxs = _draw(members, 32, 9)
    eager = [twins.train_step_on_indices(rings, idxs).clone() for _ in range(3)]
    sweep.train_step_on_indices(rings, idxs)  # warm-up: workspaces, kernel attributes (step 1 of 3)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    state = [x for m in members for t in range(2) for x in (m.trainer.flat[t], m.trainer.exp_avg[t], m.trainer.exp_avg_sq[t], m.trainer.step_count[t])]
    images = [n.packed for m in members for n in (m.policy.fused_imposter, m.policy.fused_crew)]
    saved = [x.clone() for x in state + images]
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = sweep.train_step_on_indices(rings, idxs)
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip(state + images, saved):  # (capturing runs nothing; restore in case the runtime did)
        x.copy_(sv)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[2])
    _assert_same(members)


def test_refusals_leave_the_parameters_untouched(pkg):
    L = pkg._lib
    members = _members_1v2(pkg, K=2)
    lib, stream = members[0].env.lib, members[0].env._stream()
    idxs = _draw(members, 16, 3)
    before = [m.trainer.flat[t].clone() for m in members for t in range(2)]

    def ios_of(idx_list=idxs, members_=members):
        ios, envs = (L.DqnIO * len(members_))(), (C.c_void_p * len(members_))()
        for k, m in enumerate(members_):
            ios[k], envs[k] = m.trainer._hip_io(m.ring, idx_list[k]), m.env._h
        return ios, envs

    def refused(ios, envs, n, *words):
        assert lib.susnet_dqn_train_sweep(envs, ios, n, stream) == L.E_INVALID
        msg = lib.susnet_last_error()
        assert all(w in msg for w in words), msg

    ios, envs = ios_of()
    refused(ios, envs, 0, b"n_learners")
    refused(ios, envs, 17, b"n_learners")
    ios, envs = ios_of([idxs[0], idxs[1][:8].contiguous()])
    refused(ios, envs, 2, b"learner 1", b"n differs")
    ios, envs = ios_of()
    ios[1].team[0].dims[1] = 128
    refused(ios, envs, 2, b"learner 1", b"team[0].dims")
    ios, envs = ios_of()
    ios[1].team[1].enabled = 0
    refused(ios, envs, 2, b"learner 1", b"team[1].enabled")
    # differing components: a 1v1 member whose own io is valid
    other = Member(pkg, _env_1v1(pkg, 5, ["onehot_pos"]), ["onehot_pos"], 0, False, 0.9, 1e-3)
    ios, envs = ios_of([idxs[0], idxs[1] % other.ring.size], [members[0], other])
    refused(ios, envs, 2, b"learner 1")
    same_game = Member(pkg, _env_1v1(pkg, 6, ["coord_pos"]), ["coord_pos"], 0, False, 0.9, 1e-3)
    io2, env2 = ios_of([idxs[0] % other.ring.size, idxs[1] % other.ring.size], [other, same_game])
    refused(io2, env2, 2, b"learner 1", b"components")
    ios, envs = ios_of()
    ios[1].n_components = 3
    ios[1].components[2] = L.FLAT_COMPONENTS["l1_crew"]  # (refused by learner 1's own check: no compiled-in writer)
    refused(ios, envs, 2, b"learner 1")
    ios, envs = ios_of()
    ios[1].team[0].params = ios[0].team[0].params
    refused(ios, envs, 2, b"learner 1", b"team[0].params", b"shared with learner 0")
    ios, envs = ios_of()
    ios[1].workspace, ios[1].workspace_bytes = ios[0].workspace, ios[0].workspace_bytes
    refused(ios, envs, 2, b"learner 1", b"workspace")
    torch.cuda.synchronize()
    after = [m.trainer.flat[t] for m in members for t in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    # and the unmodified table is served
    ios, envs = ios_of()
    assert lib.susnet_dqn_train_sweep(envs, ios, 2, stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(members[0].trainer.flat[0], before[0])


# ---- the loop ----
def _loop_member(pkg, seed, gamma, save_dir):
    comps = ["onehot_pos"]
    env = _env_1v1(pkg, seed, comps, batch=64)
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=seed)
    policy = pkg.PolicyRollout(env, imp, None, comps)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, None, comps, 1e-3, gamma, train_crew=False, policy=policy)
    ring = pkg.DeviceReplayBuffer(64 * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 4)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return (env, pkg.EpisodicMetricHandler(), ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.05, 100), save_dir, g)


def test_train_sweep_matches_separate_train_runs(pkg, tmp_path):
    kw = dict(train_step_interval=5, batch_size=8, num_saves=5, target_update_interval=10)
    gammas = (0.9, 0.8)
    members = [_loop_member(pkg, 60 + k, g, tmp_path / f"sweep{k}") for k, g in enumerate(gammas)]
    logs = pkg.train_sweep(members, 23, **kw)
    assert len(logs) == 2
    for k, g in enumerate(gammas):
        env, metrics, ring, policy, trainer, sched, save_dir, gen = _loop_member(pkg, 60 + k, g, tmp_path / f"alone{k}")
        log = pkg.train(env, metrics, 23, ring, policy, trainer, sched, save_dir, generator=gen, **kw)
        m = members[k]
        assert torch.equal(m[4].flat[0], trainer.flat[0]) and torch.equal(m[4].exp_avg[0], trainer.exp_avg[0])
        assert float(m[4].step_count[0]) == float(trainer.step_count[0]) > 0
        for name in (pkg.SusMetrics.IMPOSTER_LOSS, pkg.SusMetrics.CREW_LOSS, pkg.SusMetrics.AVG_IMPOSTER_RETURNS, pkg.SusMetrics.AVG_CREW_RETURNS):
            assert m[1].metrics[name] == metrics.metrics[name], name
        assert len(metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS]) == 5  # train ticks 0, 5, 10, 15, 20 (train.py:402)
        ra, rb = logs[k].records(), log.records()
        assert ra.keys() == rb.keys() and ra["count"] == rb["count"] > 0
        for key in ra:
            np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
        names = sorted(p.name for p in (tmp_path / f"sweep{k}").iterdir())
        assert names == sorted(p.name for p in (tmp_path / f"alone{k}").iterdir()) and "imposter_mlp_100%.pt" in names


def test_run_sweep_writes_one_experiment_directory_per_variant(pkg, tmp_path):
    comps = ["onehot_pos"]
    common = dict(num_steps=11, imposter_model_factory=lambda env: pkg.policy.reference_imposter_mlp(env, comps, seed=1), crew_model_factory=None,
                  components=comps, replay_buffer_size=64 * 16, replay_prepopulate_steps=4, batch_size=8, train_crew=False,
                  scheduler_time_steps=100, experiment_base_dir=tmp_path)
    factory = lambda seed: _env_1v1(pkg, seed, comps, batch=64)
    handlers = pkg.run_sweep(factory, [{"gamma": 0.9, "name": "g0.9", "seed": 1}, {"gamma": 0.8, "seed": 2}], **common)
    assert len(handlers) == 2
    assert sorted(p.name for p in tmp_path.iterdir()) == ["1", "g0.9"]
    for name, gamma, handler in (("g0.9", 0.9, handlers[0]), ("1", 0.8, handlers[1])):
        (stamp,) = list((tmp_path / name).iterdir())
        config = json.loads((stamp / "config.json").read_text())
        assert config["gamma"] == gamma and config["batch_size"] == 8 and config["num_steps"] == 11
        saved = json.loads((stamp / "metrics.json").read_text())
        n_episodes = len(handler.metrics[pkg.SusMetrics.AVG_IMPOSTER_RETURNS])
        assert n_episodes > 0
        for m in (pkg.SusMetrics.AVG_IMPOSTER_RETURNS, pkg.SusMetrics.AVG_CREW_RETURNS, pkg.SusMetrics.TOTAL_TIME_STEPS, pkg.SusMetrics.IMPOSTER_WON):
            assert len(saved[m.value]) == n_episodes, m
        assert (stamp / "imposter_mlp_100%.pt").exists()
    with pytest.raises(ValueError, match="batch_size"):
        pkg.run_sweep(factory, [{"gamma": 0.9, "batch_size": 16}], **common)
