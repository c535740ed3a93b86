"""The dense train step (susnet_mlp_train_step; DeviceDQNTeamTrainer(dense=True)) on the MI355X: exact against a float64 restatement on
integer-valued networks, close to a float64 torch run on ragged and deep stacks, close to the torch path and to the fused learner on real
rings, on the reference's own fixtures, bitwise reproducible and graph-capturable, and wired through train()."""
import copy
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from train_exact import BETAS, DEV, ExactSums, abi_step, exact_net, flatten, np_train_step, split
from train_fixtures import GOLDEN, check_final, check_first_step, mlp_from, param_names, step_indices

pytestmark = pytest.mark.gpu

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env4(pkg):
    """A 4-agent, one-imposter handle: susnet_mlp_train_step takes the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


# ---- 1. exact (the C ABI by hand, the exactness condition and the float64 restatement: tests/train_exact.py) --------------------------------
def exact_case(dims, n, seed):
    rng = np.random.default_rng(seed)
    A, M = 4, n + 7
    F, n_out = dims[0], dims[-1]
    idx = rng.permutation(M)[:n].astype(np.int64)
    imposters = np.full(M, 3, dtype=np.int16)
    imposters[idx] = np.arange(n) % 2  # agents 0 and 1 are the imposter on half the rows each, agents 2 and 3 on none
    dones = np.zeros(M, dtype=np.uint8)
    dones[idx[rng.permutation(n)[:n // 4]]] = 1
    batch = dict(feat=(rng.random((n, F)) < 0.2).astype(np.float64), next_feat=(rng.random((n, F)) < 0.2).astype(np.float64), idx=idx,
                 actions=rng.integers(0, n_out, (M, A)), rewards=rng.integers(-3, 4, (M, A)).astype(np.float64), dones=dones, imposters=imposters)
    nets = [(exact_net(rng, dims), exact_net(rng, dims)) for _ in range(2)]  # per team (online, target)
    pos = np.arange(n)
    lists = [[(a, pos[imposters[idx] == a]) for a in range(A)], [(a, pos[imposters[idx] != a]) for a in range(A)]]
    assert [len(r) for _, r in lists[0]] == [n // 2, n // 2, 0, 0] and [len(r) for _, r in lists[1]] == [n // 2, n // 2, n, n]
    return batch, nets, lists


EXACT_STACKS = [[4, 7], [78, 33, 31, 5], [131, 33, 31, 5], [36, 256, 128, 64, 16, 6], [88, 256, 128, 64, 16, 7], [1024, 256, 32]]
EXACT_CASES = [(d, n) for d in EXACT_STACKS for n in (32, 64)] + [([78, 33, 31, 5], 16384)]


@pytest.mark.parametrize("dims,n", EXACT_CASES, ids=[f"{'-'.join(map(str, d))}@{n}" for d, n in EXACT_CASES])
def test_exact_against_float64_restatement(pkg, env4, dims, n):
    """lr = 0 (the weights never move), beta1 = 0 (exp_avg after the call IS the accumulated gradient), gamma = 0.5, slopes 0.5: every sum
    of the step is exact in float32 in any order -- asserted here on the restatement -- so exp_avg must EQUAL the float64 result."""
    batch, nets, lists = exact_case(dims, n, seed=1)
    nl = len(dims) - 1
    slopes = [0.5] * (nl - 1)
    ex = ExactSums()
    want = [np_train_step(dims, nets[t][0], nets[t][1], batch, lists[t], 0.5, ex) for t in range(2)]
    print(f"exactness: worst sum|term|/q = 2^{math.log2(max(ex.worst, 1.0)):.1f}; loss sums exact: {[w[3] for w in want]}")
    assert ex.ok, f"the construction does not make every summation order exact: sum|term|/q reaches 2^{math.log2(ex.worst):.1f}"
    teams = [dict(dims=dims, params=flatten(*nets[t][0], slopes), target=flatten(*nets[t][1], slopes), lr=0.0, betas=(0.0, 0.999)) for t in range(2)]
    losses, got = abi_step(pkg, env4, teams, batch, 0.5)
    for t in range(2):
        grad, loss, steps, loss_exact, info = want[t]
        assert got[t]["step"] == steps == (2, 4)[t]
        assert np.array_equal(got[t]["params"], teams[t]["params"]), "lr = 0: the weights must not move"
        for (name, g_), (_, w_) in zip(split(dims, got[t]["exp_avg"]), split(dims, grad)):
            assert np.array_equal(g_, w_), f"team {t} {name}: max |diff| {np.abs(g_ - w_).max():.3e} of {np.abs(w_).max():.3e}"
        if loss_exact:  # (the updates' means accumulated in float32, as the step does: equal to `loss` wherever that sum is a float32 value)
            assert losses[t] == info["loss32"], (t, losses[t], info["loss32"], loss)
        else:
            np.testing.assert_allclose(losses[t], loss, rtol=1e-6)


# ---- 2. ragged and deep, against float64 -------------------------------------------------------------------------------------------------
RAGGED_STACKS = [[27, 12, 9, 8, 8, 9, 10, 5], [131, 33, 31, 5], [19, 7]]


def _double_reference(pkg, dims_pair, batch, gamma, lr, seed):
    """torch_train_step on .double() CPU modules: (models, flat params per team, losses, exp_avg per team, steps)."""
    A = batch["actions"].shape[1]
    models = []
    for t, dims in enumerate(dims_pair):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed + t)
            models.append(pkg.MLP(dims))
    init = [torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy().copy() for m in models]
    idx = torch.as_tensor(batch["idx"])
    z = torch.zeros(len(idx), 1, 1)

    def run(dtype):
        ms = [copy.deepcopy(m).to(dtype) for m in models]
        ts = [copy.deepcopy(m) for m in ms]
        opts = [torch.optim.Adam(m.parameters(), lr=lr) for m in ms]
        fs, fn = (torch.as_tensor(batch[k]).to(dtype).unsqueeze(1) for k in ("feat", "next_feat"))
        losses = pkg.torch_train_step(ms, ts, opts, gamma, [(z.to(dtype), fs)] * A, [(z.to(dtype), fn)] * A, torch.as_tensor(batch["actions"])[idx].long(),
                                      torch.as_tensor(batch["rewards"])[idx].to(dtype), torch.as_tensor(batch["dones"])[idx].bool().reshape(-1, 1),
                                      torch.as_tensor(batch["imposters"])[idx].to(torch.int16).reshape(-1, 1))
        ea, steps = [], []
        for m, o in zip(ms, opts):
            ea.append(np.concatenate([(o.state[p]["exp_avg"].double().numpy().reshape(-1) if p in o.state else np.zeros(p.numel())) for p in m.parameters()]))
            steps.append(float(next(iter(o.state.values()))["step"]) if o.state else 0.0)
        return np.asarray(losses, dtype=np.float64), ea, steps

    return init, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("n", [1, 31, 33, 65])
@pytest.mark.parametrize("dims", RAGGED_STACKS, ids=["7layers", "131-33-31-5", "19-7"])
def test_ragged_and_deep_against_float64(pkg, env4, dims, n):
    """Random float weights, ragged tiles (n = 1, 31, 33, 65), units and k; the reference is torch_train_step on float64 CPU copies.
    Tolerances are the project's: losses rtol 1e-4, the first step's gradient (exp_avg / (1 - beta1)) within 1e-4 of each tensor's
    max-abs, step counts exact.  The float32 torch path's own error against the same float64 result is printed beside the kernel's.
    Measured on an MI355X over the 240 tensors of the 12 cases: the kernel within 3.6e-5 of max-abs (float32 torch: 3.9e-5), losses within
    1.2e-7 relative (float32 torch: 1.3e-7) -- no case needed more than the tolerances above."""
    rng = np.random.default_rng(100 + n)
    A, M, F = 4, n + 5, dims[0]
    crew_dims = dims[:-1] + [dims[-1] + 2]
    batch = dict(feat=rng.random((n, F)).round(3) * (rng.random((n, F)) < 0.5), next_feat=rng.random((n, F)).round(3) * (rng.random((n, F)) < 0.5),
                 idx=rng.integers(0, M, n).astype(np.int64), actions=rng.integers(0, dims[-1], (M, A)), rewards=rng.normal(size=(M, A)).astype(np.float32),
                 dones=(rng.random(M) < 0.3).astype(np.uint8), imposters=rng.integers(0, A, M).astype(np.int16))
    batch["feat"], batch["next_feat"] = batch["feat"].astype(np.float32), batch["next_feat"].astype(np.float32)
    init, (l64, ea64, st64), (l32, ea32, _) = _double_reference(pkg, (dims, crew_dims), batch, 0.9, 1e-3, seed=n)
    teams = [dict(dims=d, params=init[t], target=init[t], lr=1e-3, betas=BETAS) for t, d in enumerate((dims, crew_dims))]
    losses, got = abi_step(pkg, env4, teams, batch, 0.9)
    for t, d in enumerate((dims, crew_dims)):
        assert got[t]["step"] == st64[t]
        for (name, g_), (_, r_), (_, f_) in zip(split(d, got[t]["exp_avg"]), split(d, ea64[t]), split(d, ea32[t])):
            scale = max(float(np.abs(r_).max()), 1e-30)
            err, err32 = float(np.abs(g_ - r_).max()) / scale, float(np.abs(f_ - r_).max()) / scale
            print(f"team {t} {name}: kernel {err:.2e}, float32 torch {err32:.2e} of max-abs")
            assert err <= 1e-4 or float(np.abs(r_).max()) == 0.0 == float(np.abs(g_).max()), f"team {t} {name}: first-step gradient off by {err:.2e}"
    print(f"losses: kernel rel {np.abs(losses - l64) / np.maximum(np.abs(l64), 1e-30)}, float32 torch rel {np.abs(l32 - l64) / np.maximum(np.abs(l64), 1e-30)}")
    np.testing.assert_allclose(losses, l64, rtol=1e-4)


# ---- 3. / 4. against the torch path and the fused learner on real rings -------------------------------------------------------------------
def base_1v3(pkg, batch, **kw):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9, shuffle_imposter_index=True,
                                  obs=pkg.ObsConfig("flat", COMPS3), **kw)


def tagging_1v4(pkg, batch, **kw):
    return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=4, auto_reset=True, grid_size=9,
                                             obs=pkg.ObsConfig("flat", ["onehot_pos"]), **kw)


def game_1v2(pkg, batch):
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device=DEV, rng="philox", seed=5, auto_reset=True, grid_size=14, shuffle_imposter_index=True)


@pytest.fixture(scope="module")
def rings(pkg):
    """game -> (env, components, crew trained, ring): populate_fused with batch 256 x 8 ticks, made once."""
    out = {}
    for game, env, comps, crew in (("base_1v3", base_1v3(pkg, 256), COMPS3, True), ("tagging_1v4", tagging_1v4(pkg, 256), ["onehot_pos"], False),
                                   ("base14_1v2", game_1v2(pkg, 256), COMPS3, True)):
        ring = pkg.DeviceReplayBuffer(256 * 8, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
        ring.populate_fused(env, 8)
        out[game] = (env, comps, crew, ring)
    return out


def _split_params(tr, t, flat):
    out, off = [], 0
    for p in tr.models[t].parameters():
        out.append(flat[off:off + p.numel()])
        off += p.numel()
    return out


def _compare_two_steps(a, b, ring, n):
    """test_gpu_train.py::test_hip_matches_torch_path's comparison of trainer `a` (under test) with `b`: losses rtol 1e-4 / atol 1e-6, the
    first step's exp_avg per tensor within 1e-4 of its max-abs, step counts equal, the two-step movement within 2e-2."""
    init = [f.clone() if f is not None else None for f in a.flat]
    g = torch.Generator(device=DEV)
    g.manual_seed(n)
    for k in range(2):
        idx = torch.randint(0, ring.size, (n,), device=DEV, generator=g)
        la = a.train_step_on_indices(ring, idx).clone()
        lb = b.train_step_on_indices(ring, idx)
        torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-6)
        for t in range(2):
            if not a.trained[t]:
                continue
            ea, _, sa = a.state_tensors(t)
            eb, _, sb = b.state_tensors(t)
            assert float(sa) == float(sb) > 0
            if k == 0:
                for (name, _), x, y in zip(a.models[t].named_parameters(), _split_params(a, t, ea), _split_params(a, t, eb)):
                    assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-12, name
    for t in range(2):
        if a.trained[t]:
            rel = float((a.flat[t] - b.flat[t]).norm() / (b.flat[t] - init[t]).norm())
            assert rel <= 2e-2, rel


@pytest.mark.parametrize("n", [8, 32, 4096])
@pytest.mark.parametrize("game", ["base_1v3", "tagging_1v4"])
def test_dense_matches_torch_path(pkg, rings, game, n):
    env, comps, crew, ring = rings[game]
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    cr = pkg.policy.reference_crew_mlp(env, comps, seed=4) if crew else None
    dense = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-3, 0.9, train_crew=crew, dense=True)
    ref = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, 1e-3, 0.9, train_crew=crew)
    assert dense.uses_dense(ring) and not dense.uses_hip(ring)
    assert not ref.uses_dense(ring) and not ref.uses_hip(ring)
    _compare_two_steps(dense, ref, ring, n)


@pytest.mark.parametrize("n", [32, 4096])
def test_dense_matches_the_fused_learner(pkg, rings, n):
    """Two independent kernels on the 1v2 14x14 layout: the dense step (the fused one switched off by hand) and susnet_dqn_train_step."""
    env, comps, _, ring = rings["base14_1v2"]
    imp, cr = pkg.policy.reference_imposter_mlp(env, comps, seed=3), pkg.policy.reference_crew_mlp(env, comps, seed=4)
    dense = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-3, 0.9, dense=True)
    fused = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, 1e-3, 0.9)
    assert fused.uses_hip(ring) and dense.uses_hip(ring) and not dense.uses_dense(ring), "the compiled-in layouts keep the fused step"
    dense.hip = False
    assert dense.uses_dense(ring) and not dense.uses_hip(ring)
    _compare_two_steps(dense, fused, ring, n)


# ---- 5. the reference's own train_step (tests/golden/dense/dense_train_*.npz, generate_train_dense.py) ---------------------------------------------
@pytest.mark.parametrize("name", ["base9_1v3_j5_comps3", "base9_1v3_j5_coord_deep"])
def test_dense_step_reproduces_reference_fixture(pkg, name):
    d = np.load(os.path.join(GOLDEN, "dense", f"dense_train_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    comps = meta["components"]
    k = dict(meta["kwargs"])
    env = pkg.BatchedFourRoomEnv(k.pop("n_imposters"), k.pop("n_crew"), k.pop("n_jobs"), grid=np.array(meta["grid"], dtype=bool), **k, batch=64,
                                 device=DEV, rng="philox", seed=1, auto_reset=True, obs=pkg.ObsConfig("flat", comps))
    M = d["ring::states"].shape[0]
    ring = pkg.DeviceReplayBuffer(M, meta["state_size"], 1, meta["n_agents"], meta["n_imposters"], device=DEV)
    for key in ("states", "next_states", "actions", "rewards", "dones", "imposters"):
        dst = getattr(ring, key)
        dst.copy_(torch.tensor(d["ring::" + key]).reshape(dst.shape).to(dst.dtype))
    ring.size = ring.idx = M
    imp = mlp_from(pkg, d, "imposter", meta["imposter_dims"]).to(DEV)
    crew = mlp_from(pkg, d, "crew", meta["crew_dims"]).to(DEV)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, crew, comps, meta["lr"], meta["gamma"], dense=True)
    assert tr.uses_dense(ring) and not tr.uses_hip(ring)
    models = [imp, crew]
    for step, idx in enumerate(step_indices(meta, d)):
        losses = tr.train_step_on_indices(ring, torch.tensor(idx, device=DEV)).cpu().numpy()
        np.testing.assert_allclose(losses, d["losses"][step], rtol=1e-4, atol=1e-7)
        if step == 0:
            for t, team in enumerate(("imposter", "crew")):
                named = dict(models[t].named_parameters())
                ea = {n: v.view_as(named[n]).cpu().numpy() for n, v in zip(named, _split_params(tr, t, tr.state_tensors(t)[0]))}
                check_first_step(d, team, {n: ea[n] for n in param_names(d, team)})
    for t, team in enumerate(("imposter", "crew")):
        named = dict(models[t].named_parameters())
        check_final(d, team, {n: named[n].detach().cpu().numpy() for n in param_names(d, team)}, float(tr.state_tensors(t)[2]))


# ---- 6. determinism and capture ----------------------------------------------------------------------------------------------------------
def _state(tr):
    return [x for t in range(2) if tr.trained[t] for x in (tr.flat[t], tr.exp_avg[t], tr.exp_avg_sq[t], tr.step_count[t])]


def test_bitwise_deterministic(pkg, rings):
    env, comps, _, ring = rings["base_1v3"]
    imp, cr = pkg.policy.reference_imposter_mlp(env, comps, seed=3), pkg.policy.reference_crew_mlp(env, comps, seed=4)
    a = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-3, 0.9, dense=True)
    b = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, 1e-3, 0.9, dense=True)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    for n in (4096, 33, 4096):
        idx = torch.randint(0, ring.size, (n,), device=DEV, generator=g)
        la, lb = a.train_step_on_indices(ring, idx).clone(), b.train_step_on_indices(ring, idx).clone()
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all()) and float(la.sum()) > 0
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y)


def test_graph_replay_matches_eager(pkg):
    env = tagging_1v4(pkg, 256, check_errors=False, export_state=False)
    ring = pkg.DeviceReplayBuffer(256 * 4, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 4)
    imp = pkg.policy.reference_imposter_mlp(env, ["onehot_pos"], seed=3)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, None, ["onehot_pos"], 1e-3, 0.9, dense=True)
    assert tr.uses_dense(ring)
    idx = torch.randint(0, ring.size, (64,), device=DEV)
    tr.train_step_on_indices(ring, idx)  # one eager step first: buffers, workspace, kernel attributes
    torch.cuda.synchronize()
    saved = [x.clone() for x in _state(tr)]
    eager_losses = [tr.train_step_on_indices(ring, idx).clone() for _ in range(3)]
    eager = [x.clone() for x in _state(tr)]
    for x, s in zip(_state(tr), saved):
        x.copy_(s)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = tr.train_step_on_indices(ring, idx)
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip(_state(tr), saved):
        x.copy_(sv)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_losses[k]), k
    for x, e in zip(_state(tr), eager):
        assert torch.equal(x, e)


# ---- 7. wiring ---------------------------------------------------------------------------------------------------------------------------
def test_train_runs_on_the_dense_step(pkg, tmp_path):
    B, num_steps, k, batch_size = 64, 32, 4, 16
    env = tagging_1v4(pkg, B, max_time_steps=20)
    comps = ["onehot_pos"]
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    policy = pkg.PolicyRollout(env, imp, None, components=comps, mask_dead=True, dense=True)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, None, comps, lr=1e-3, gamma=0.9, policy=policy, dense=True)
    ring = pkg.DeviceReplayBuffer(B * num_steps, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    assert policy.dense_imposter is not None and trainer.uses_dense(ring) and not trainer.uses_hip(ring)
    before = [p.detach().clone() for p in imp.parameters()]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    metrics = pkg.EpisodicMetricHandler()
    pkg.train(env, metrics, num_steps, ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.05, 30), tmp_path / "run", train_step_interval=k,
              batch_size=batch_size, generator=gen)
    losses = metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS]
    assert len(losses) == 1 + (num_steps - 1) // k
    assert all(math.isfinite(v) for v in losses) and any(v > 0 for v in losses)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, imp.parameters()))
    # the policy reads the parameters in place: no refresh call was needed
    q, _ = policy.q_rows()
    with torch.no_grad():
        want = imp(policy._spatial, env.obs)
    torch.testing.assert_close(q, want, rtol=0, atol=2e-5 * float(want.abs().max()))
    # the optimizer state round-trips through torch's format
    steps = float(trainer.state_tensors(0)[2])  # (one Adam step per agent that is the imposter somewhere in the batch)
    assert len(losses) <= steps <= len(losses) * env.n_agents
    sd = trainer.optimizer_state_dict(0)
    opt = torch.optim.Adam(copy.deepcopy(imp).parameters(), lr=1e-3)
    opt.load_state_dict(sd)
    assert float(sd["state"][0]["step"]) == steps
    other = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), None, comps, lr=1e-3, gamma=0.9, dense=True)
    other.target_flat[0].copy_(trainer.target_flat[0])
    other.load_optimizer_state_dict(0, sd)
    idx = torch.randint(0, ring.size, (batch_size,), device=DEV, generator=gen)
    u = len(set(ring.imposters[idx].reshape(-1).tolist()))  # this batch's non-empty updates
    la, lb = trainer.train_step_on_indices(ring, idx).clone(), other.train_step_on_indices(ring, idx).clone()
    assert torch.equal(la, lb) and torch.equal(trainer.flat[0], other.flat[0]) and torch.equal(trainer.exp_avg[0], other.exp_avg[0])
    # switching to the torch path mid-run and back keeps the step counts
    other.dense = False
    assert not other.uses_dense(ring)
    other.train_step_on_indices(ring, idx)
    assert float(other.optimizer_state_dict(0)["state"][0]["step"]) == steps + 2 * u
    other.dense = True
    other.train_step_on_indices(ring, idx)
    assert float(other.state_tensors(0)[2]) == steps + 3 * u and bool(torch.isfinite(other.flat[0]).all())


def test_defaults_are_unchanged(pkg, rings):
    env, comps, _, ring = rings["tagging_1v4"]
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, None, comps, 1e-3, 0.9)
    assert not tr.dense and not tr.uses_dense(ring) and not tr.uses_hip(ring)
    import inspect
    assert inspect.signature(pkg.run_experiment).parameters["dense_train"].default is False
    assert inspect.signature(pkg.run_sweep).parameters["dense_train"].default is False
