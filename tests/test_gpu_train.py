"""The device train step (susnet_dqn_train_step, DeviceDQNTeamTrainer) against the torch path of the same algorithm
(DQNTeamTrainer.train_step, src/train.py:50-149), on the MI355X."""
import copy
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _game_1v2(pkg, batch=1024, obs=None):
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=5, auto_reset=True, grid_size=14,
                                  shuffle_imposter_index=True, **({"obs": obs} if obs is not None else {}))


def _game_1v1(pkg, batch=1024, obs=None):
    kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
    return pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device="cuda:0", rng="philox", seed=6,
                                             auto_reset=True, **({"obs": obs} if obs is not None else {}))


def _ring(pkg, env, ticks=16, T=1):
    ring = pkg.DeviceReplayBuffer(env.batch * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, ticks)
    return ring


def _models(pkg, env, comps, crew=True):
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    cr = pkg.policy.reference_crew_mlp(env, comps, seed=4) if crew else None
    return imp, cr


def _split(tr, t, flat):
    out, off = [], 0
    for p in tr.models[t].parameters():
        out.append(flat[off:off + p.numel()])
        off += p.numel()
    return out


def _pair(pkg, env, comps, crew=True, lr=1e-3, gamma=0.9):
    imp, cr = _models(pkg, env, comps, crew)
    hip = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, lr, gamma, train_crew=crew)
    ref = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, lr, gamma, train_crew=crew)
    ref.hip = False
    return hip, ref


@pytest.mark.parametrize("game", ["1v2", "1v1"])
@pytest.mark.parametrize("n", [8, 32, 4096, 65536])
def test_hip_matches_torch_path(pkg, game, n):
    env = _game_1v2(pkg) if game == "1v2" else _game_1v1(pkg)
    comps = COMPS3 if game == "1v2" else ["onehot_pos"]
    ring = _ring(pkg, env)
    hip, ref = _pair(pkg, env, comps, crew=game == "1v2")
    assert hip.uses_hip(ring) and not ref.uses_hip(ring)
    init = [f.clone() if f is not None else None for f in hip.flat]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(n)
    for k in range(2):
        idx = torch.randint(0, ring.size, (n,), device="cuda:0", generator=g)
        lh = hip.train_step_on_indices(ring, idx).clone()
        lr_ = ref.train_step_on_indices(ring, idx)
        torch.testing.assert_close(lh, lr_, rtol=1e-4, atol=1e-6)
        for t in range(2):
            if not hip.trained[t]:
                continue
            eh, _, sh = hip.state_tensors(t)
            er, _, sr = ref.state_tensors(t)
            assert float(sh) == float(sr)
            if k == 0:  # first step: exp_avg = (1 - beta1) g, per tensor
                for (name, _), a_, r_ in zip(hip.models[t].named_parameters(), _split(hip, t, eh), _split(hip, t, er)):
                    assert float((a_ - r_).abs().max()) <= 1e-4 * float(r_.abs().max()) + 1e-12, name
    for t in range(2):
        if hip.trained[t]:
            rel = float((hip.flat[t] - ref.flat[t]).norm() / (ref.flat[t] - init[t]).norm())
            assert rel <= 2e-2, rel


def test_bitwise_deterministic_and_packed_image(pkg):
    env = _game_1v2(pkg, obs=pkg.ObsConfig("flat", COMPS3))
    ring = _ring(pkg, env)
    imp, cr = _models(pkg, env, COMPS3)
    policy = pkg.PolicyRollout(env, imp, cr, COMPS3)
    a = pkg.DeviceDQNTeamTrainer(env, imp, cr, COMPS3, 1e-3, 0.9, policy=policy)
    b = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), COMPS3, 1e-3, 0.9)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    for _ in range(3):
        idx = torch.randint(0, ring.size, (4096,), device="cuda:0", generator=g)
        la = a.train_step_on_indices(ring, idx).clone()
        lb = b.train_step_on_indices(ring, idx).clone()
        assert torch.equal(la, lb)
        for t in range(2):
            assert torch.equal(a.flat[t], b.flat[t]) and torch.equal(a.exp_avg[t], b.exp_avg[t]) and torch.equal(a.exp_avg_sq[t], b.exp_avg_sq[t])
        # the device-rewritten images are bitwise the host packer's on the modules' parameters
        for model, net in ((imp, policy.fused_imposter), (cr, policy.fused_crew)):
            fresh = pkg.policy.pack_mlp(env, model, COMPS3)
            assert torch.equal(net.packed, fresh.packed)
        assert policy.refresh_weights(force=False) is False
        # the policy acts with the new weights, with no host re-pack
        q_imp, q_crew = policy.q_rows()
        assert torch.equal(q_imp, env.qnet_forward(pkg.policy.pack_mlp(env, imp, COMPS3)))
        assert torch.equal(q_crew, env.qnet_forward(pkg.policy.pack_mlp(env, cr, COMPS3)))


def test_graph_replay_matches_eager(pkg):
    env = _game_1v1(pkg)
    ring = _ring(pkg, env)
    imp, _ = _models(pkg, env, ["onehot_pos"], crew=False)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, None, ["onehot_pos"], 1e-3, 0.9)
    idx = torch.randint(0, ring.size, (32,), device="cuda:0")
    tr.train_step_on_indices(ring, idx)  # warm-up: workspace, kernel attributes
    torch.cuda.synchronize()
    saved = [x.clone() for x in (tr.flat[0], tr.exp_avg[0], tr.exp_avg_sq[0], tr.step_count[0])]
    eager_loss = tr.train_step_on_indices(ring, idx).clone()
    eager = [x.clone() for x in (tr.flat[0], tr.exp_avg[0], tr.exp_avg_sq[0], tr.step_count[0])]
    for x, s in zip((tr.flat[0], tr.exp_avg[0], tr.exp_avg_sq[0], tr.step_count[0]), saved):
        x.copy_(s)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = tr.train_step_on_indices(ring, idx)
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip((tr.flat[0], tr.exp_avg[0], tr.exp_avg_sq[0], tr.step_count[0]), saved):
        x.copy_(sv)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_loss)
    for x, e in zip((tr.flat[0], tr.exp_avg[0], tr.exp_avg_sq[0], tr.step_count[0]), eager):
        assert torch.equal(x, e)


def test_unserved_configurations_are_refused_by_the_library(pkg):
    import ctypes as C

    L = pkg._lib
    env = _game_1v2(pkg, batch=256)
    imp, cr = _models(pkg, env, COMPS3)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, cr, COMPS3, 1e-3, 0.9)
    assert tr.hip
    # a ring window of two states with a served network: the library refuses it, and the trainer does not route it there
    ring2 = _ring(pkg, env, ticks=4, T=2)
    assert not tr.uses_hip(ring2)
    idx = torch.randint(0, ring2.size, (32,), device="cuda:0")
    io = tr._io(ring2, idx)
    nbytes = C.c_uint64()
    assert env.lib.susnet_dqn_workspace_bytes(env._h, C.byref(io), C.byref(nbytes)) == L.E_INVALID
    assert b"trajectory_size" in env.lib.susnet_last_error()
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda:0")
    losses = torch.zeros(2, device="cuda:0")
    io.workspace, io.workspace_bytes, io.losses_out = ws.data_ptr(), ws.numel(), losses.data_ptr()
    assert env.lib.susnet_dqn_train_step(env._h, C.byref(io), env._stream()) == L.E_INVALID
    # two imposters: refused by the library (citing the reference line) and by the trainer
    env2 = pkg.BatchedFourRoomEnv(2, 3, 4, batch=64, device="cuda:0", rng="philox", seed=1, auto_reset=True, grid_size=14)
    ring1 = _ring(pkg, env, ticks=2)
    io = tr._io(ring1, idx % ring1.size)
    assert env2.lib.susnet_dqn_workspace_bytes(env2._h, C.byref(io), C.byref(nbytes)) == L.E_INVALID
    assert b"train.py:83" in env2.lib.susnet_last_error()
    with pytest.raises(ValueError, match="train.py:83"):
        pkg.DeviceDQNTeamTrainer(env2, pkg.MLP([10, 8, 8, 8, 8, 5]), None, ["onehot_pos"], 1e-3, 0.9)
    # a policy reading another feature layout than the trainer: refused (its image would be rewritten in the wrong layout)
    env_c = _game_1v1(pkg, batch=256, obs=pkg.ObsConfig("flat", ["coord_pos"]))
    m = pkg.policy.reference_imposter_mlp(env_c, ["coord_pos"], seed=3)
    pol = pkg.PolicyRollout(env_c, m, None, ["coord_pos"])
    with pytest.raises(ValueError, match="components"):
        pkg.DeviceDQNTeamTrainer(env_c, m, None, ["onehot_pos"], 1e-3, 0.9, policy=pol)


def test_spatial_dqn_trains_through_the_torch_path(pkg):
    env = _game_1v2(pkg, batch=256)
    ring = _ring(pkg, env, ticks=4)
    fz = pkg.GlobalFeaturizer(env)
    fz.fit(ring.states[:2])
    sp0, ns0 = fz.generate_featurized_states()[0]
    C_, N_ = sp0.shape[2], sp0.shape[3]
    torch.manual_seed(0)
    sp = pkg.SpatialDQN(N_, ns0.shape[-1], [C_], [1], [0], (3, 3), [1], 1, 16, 0.0, [16], env.n_imposter_actions).cuda()
    ref_model = copy.deepcopy(sp)
    ref_target = ref_model.create_copy().cuda()
    tr = pkg.DeviceDQNTeamTrainer(env, sp, None, COMPS3, 1e-3, 0.9, featurizer=pkg.GlobalFeaturizer(env))
    assert not tr.hip
    idx = torch.randint(0, ring.size, (64,), device="cuda:0")
    losses = tr.train_step_on_indices(ring, idx)
    fz.fit(ring.states[idx])
    sf = fz.generate_featurized_states()
    fz.fit(ring.next_states[idx])
    nf = fz.generate_featurized_states()
    opt = torch.optim.Adam(ref_model.parameters(), lr=1e-3)
    expect = pkg.torch_train_step([ref_model, None], [ref_target, None], [opt, None], 0.9, sf, nf, ring.actions[idx], ring.rewards[idx],
                                  ring.dones[idx], ring.imposters[idx])
    assert float(losses[0]) == pytest.approx(expect[0], rel=1e-5)
    for p, q in zip(sp.parameters(), ref_model.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)


def test_optimizer_state_round_trip_path_switch_and_target_sync(pkg):
    env = _game_1v1(pkg)
    ring = _ring(pkg, env)
    imp, _ = _models(pkg, env, ["onehot_pos"], crew=False)
    a = pkg.DeviceDQNTeamTrainer(env, imp, None, ["onehot_pos"], 1e-3, 0.9)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    idx = [torch.randint(0, ring.size, (64,), device="cuda:0", generator=g) for _ in range(4)]
    a.train_step_on_indices(ring, idx[0])
    a.train_step_on_indices(ring, idx[1])
    sd = a.optimizer_state_dict(0)
    # a real torch.optim.Adam takes it and holds the same moments
    m2 = copy.deepcopy(imp)
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    opt.load_state_dict(sd)
    for i, p in enumerate(m2.parameters()):
        assert torch.equal(opt.state[p]["exp_avg"], sd["state"][i]["exp_avg"]) and float(opt.state[p]["step"]) == 2.0
    # a second trainer loaded from it continues bitwise like the first
    b = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), None, ["onehot_pos"], 1e-3, 0.9)
    b.target_flat[0].copy_(a.target_flat[0])
    b.load_optimizer_state_dict(0, sd)
    a.train_step_on_indices(ring, idx[2])
    b.train_step_on_indices(ring, idx[2])
    assert torch.equal(a.flat[0], b.flat[0]) and torch.equal(a.state_tensors(0)[0], b.state_tensors(0)[0])
    # switching paths mid-run carries the Adam state both ways
    b.hip = False
    b.train_step_on_indices(ring, idx[3])
    assert float(b.optimizer_state_dict(0)["state"][0]["step"]) == 4.0
    b.hip = True
    b.train_step_on_indices(ring, idx[3])
    assert float(b.state_tensors(0)[2]) == 5.0 and bool(torch.isfinite(b.flat[0]).all())
    # the target update of train.py:341-343
    assert not torch.equal(a.target_flat[0], a.flat[0])
    a.sync_targets()
    for p, q in zip(a.targets[0].parameters(), a.models[0].parameters()):
        assert torch.equal(p, q)


# ---- the HIP path against the reference's own train_step (tests/golden/model_train_*.npz, generate_train.py) ----
from train_fixtures import check_final, check_first_step, fixture_names, load, mlp_from, param_names, step_indices  # noqa: E402


def _fixture_env(pkg, meta, comps):
    kw = dict(batch=64, device="cuda:0", rng="philox", seed=1, auto_reset=True, obs=pkg.ObsConfig("flat", comps))
    if meta["class"] == "itg":
        return pkg.BatchedImposterTrainingGround(**meta["kwargs"], **kw)
    k = dict(meta["kwargs"])
    return pkg.BatchedFourRoomEnv(k.pop("n_imposters"), k.pop("n_crew"), k.pop("n_jobs"), grid=np.array(meta["grid"], dtype=bool), **k, **kw)


@pytest.mark.parametrize("name", fixture_names())
def test_hip_path_reproduces_reference_fixture(pkg, name):
    meta, d = load(name)
    comps = meta["components"]
    env = _fixture_env(pkg, meta, comps)
    M = d["ring::states"].shape[0]
    ring = pkg.DeviceReplayBuffer(M, meta["state_size"], 1, meta["n_agents"], meta["n_imposters"], device="cuda:0")
    for k in ("states", "next_states", "actions", "rewards", "dones", "imposters"):
        dst = getattr(ring, k)
        dst.copy_(torch.tensor(d["ring::" + k]).reshape(dst.shape).to(dst.dtype))
    ring.size = ring.idx = M
    trained = [meta["train_imposter"], meta["train_crew"]]
    imp = mlp_from(pkg, d, "imposter", meta["imposter_dims"]).cuda()
    crew = mlp_from(pkg, d, "crew", meta["crew_dims"]).cuda()
    crew_arg = crew if trained[1] else None
    policy = pkg.PolicyRollout(env, imp, crew_arg, comps)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, crew_arg, comps, meta["lr"], meta["gamma"], train_imposter=trained[0], train_crew=trained[1],
                                  policy=policy)
    assert tr.uses_hip(ring)
    models = [imp, crew]
    for k, idx in enumerate(step_indices(meta, d)):
        losses = tr.train_step_on_indices(ring, torch.tensor(idx, device="cuda:0")).cpu().numpy()
        np.testing.assert_allclose(losses, d["losses"][k], rtol=1e-4, atol=1e-7)
        # the image rewritten on the device is bitwise the host packer's on the updated parameters (every layout's packer)
        for net, model in ((policy.fused_imposter, imp), (policy.fused_crew, crew)):
            if net is not None:
                assert torch.equal(net.packed, pkg.policy.pack_mlp(env, model, comps).packed)
        if k == 0:
            for t, team in enumerate(("imposter", "crew")):
                if trained[t]:
                    named = dict(models[t].named_parameters())
                    ea = {n: v.view_as(named[n]).cpu().numpy() for n, v in zip(named, _split(tr, t, tr.state_tensors(t)[0]))}
                    check_first_step(d, team, {n: ea[n] for n in param_names(d, team)})
    for t, team in enumerate(("imposter", "crew")):
        named = dict(models[t].named_parameters())
        step = float(tr.state_tensors(t)[2]) if trained[t] else 0.0
        check_final(d, team, {n: named[n].detach().cpu().numpy() for n in param_names(d, team)}, step)
