"""The SpatialDQN train step (susnet_spatial_train_step; DeviceDQNTeamTrainer(spatial=True)) on the MI355X: close to a float64 torch run on
ragged tiles and varied networks in both featurizer layouts, exact ReLU gates on integer convolutions, the step's semantics (empty lists,
done rows, accumulation over agents, n = 0), the reference's own fixtures, bitwise reproducible and graph-capturable, and wired through
the trainer.  The float64 reference throughout is torch_train_step on .double() CPU copies."""
import copy
import importlib
import inspect

import numpy as np
import pytest
import torch

from spatial_train_util import SpatialCall, as_global, compare_tensors, flat, make_batch, make_model, split, torch_reference
from train_exact import DEV

pytestmark = pytest.mark.gpu

A3, N5, C3 = 3, 5, 3  # 1v2, a hand-made 5 x 5 grid of 3 channels


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env3(pkg):
    """A 3-agent, one-imposter handle: susnet_spatial_train_step takes the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


# ---- 1. ragged and varied, against float64 ---------------------------------------------------------------------------------------------
# (n, T, Fn, imposter network, crew network); a network: (chans behind C, k, strides, pads, dils, rnn layers, hidden, head hidden widths).
# The CNN has len(chans) + 1 convolutions: the reference repeats the last entry of every list (so the last two layers share stride, padding
# and dilation and must keep the size: that is the reference's own constraint, dqn.py:155-159 against utils.py:5-11)
RAGGED = [
    (1, 1, 0, ([], 1, [1], [0], [1], 1, 5, []), ([2], 3, [1], [2], [2], 3, 5, [4])),                           # n_conv 1, k 1, no hidden | dilation 2, padding 2
    (31, 2, 4, ([4, 6, 5], 3, [1, 2, 1], [2, 1, 1], [1, 1, 1], 3, 33, [7, 6, 9]), ([], 1, [1], [0], [1], 1, 33, [])),  # n_conv 4, stride 2, 3 hidden
    (33, 8, 2, ([4], 5, [1], [2], [1], 1, 33, [8]), ([3, 2], 3, [2, 1], [0, 1], [1, 1], 3, 5, [6])),            # k 5, T 8 | stride 2 first, padding 0
    (65, 2, 3, ([], 3, [1], [0], [1], 3, 33, [5, 4, 3]), ([2], 5, [1], [2], [1], 1, 5, [])),                    # padding 0 shrinking | two blocks + 1
]


def _nets(pkg, Fn, specs, seed):
    out = []
    for t, (chans, k, strides, pads, dils, layers, hidden, head) in enumerate(specs):
        out.append(make_model(pkg, N5, C3, Fn, chans, strides, pads, k, dils, layers, hidden, head, (5, 4)[t], seed + t))
    return out


@pytest.mark.parametrize("layout", ["global", "perspective"])
@pytest.mark.parametrize("case", RAGGED, ids=[f"n{c[0]}-T{c[1]}-Fn{c[2]}" for c in RAGGED])
def test_ragged_and_varied_against_float64(pkg, env3, case, layout):
    """Random float weights on 0/1 planes; ragged tiles (the row tile is 32), both teams with different networks on the same inputs, every
    parameter tensor compared on its own.  Tolerances are the project's: losses rtol 1e-4, the first step's gradient (exp_avg, i.e.
    (1 - beta1) x the accumulated gradient after the call's updates) within 1e-4 of each tensor's max-abs, step counts exact.  The float32
    torch path's own error against the same float64 result is printed beside the kernel's.  Measured on an MI355X over the tensors of
    these cases and the other float64 tests of this file: the kernel within 3.8e-6 of max-abs (float32 torch: 2.2e-6), losses within 2.1e-7
    relative (float32 torch: 1.7e-7) -- no case needed more than the tolerances above."""
    n, T, Fn, imp, crew = case
    rng = np.random.default_rng(7 * n + T)
    models = _nets(pkg, Fn, (imp, crew), seed=n)
    batch = make_batch(rng, n, T, A3, C3, N5, Fn, 4)
    if layout == "global":
        batch = as_global(batch)
    l64, ea64, st64, _ = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float64)
    l32, ea32, _, _ = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float32)
    losses, got = SpatialCall(pkg, env3, models, models, batch, 0.9).step()
    for t in range(2):
        assert got[t]["step"] == st64[t], (t, got[t]["step"], st64[t])
        compare_tensors(models[t], got[t]["exp_avg"], ea64[t], ea32[t], f"team {t}")
    print(f"losses: kernel rel {np.abs(losses - l64[0]) / np.maximum(np.abs(l64[0]), 1e-30)}, "
          f"float32 torch rel {np.abs(l32[0] - l64[0]) / np.maximum(np.abs(l64[0]), 1e-30)}")
    np.testing.assert_allclose(losses, l64[0], rtol=1e-4)


# ---- 2. exact gates ------------------------------------------------------------------------------------------------------------------------
def test_relu_gates_on_integer_convolutions(pkg, env3):
    """Convolution weights and biases are small integers on 0/1 planes: every pre-activation is an exact integer in float32 and in float64
    and many are exactly 0 -- where ReLU passes nothing back (torch: grad where the OUTPUT is > 0).  A gate of >= 0 would let those through."""
    n, T, Fn = 33, 2, 2
    rng = np.random.default_rng(5)
    model = make_model(pkg, N5, C3, Fn, [4], [1], [1], 3, [1], 1, 9, [6], 5, seed=11)
    convs = [m for m in model.cnn.model if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        for m in convs:
            m.weight.copy_(torch.as_tensor(rng.integers(-1, 2, tuple(m.weight.shape)) * (rng.random(tuple(m.weight.shape)) < 0.5)).float())
            m.bias.copy_(torch.as_tensor(rng.integers(-1, 1, tuple(m.bias.shape))).float())
    batch = as_global(make_batch(rng, n, T, A3, C3, N5, Fn, 5, density=0.25))
    # the pre-activations of the float64 run
    x = torch.as_tensor(batch["spatial"]).double().reshape(-1, C3, N5, N5)
    zeros = total = 0
    with torch.no_grad():
        for m in convs:
            z = copy.deepcopy(m).double()(x)
            assert torch.equal(z, z.round()), "integer weights on 0/1 planes: integer pre-activations"
            zeros, total = zeros + int((z == 0).sum()), total + z.numel()
            x = torch.relu(z)
    print(f"pre-activations exactly 0: {zeros} of {total}")
    assert zeros * 10 >= total, "the case is meant to sit on the kink: at least a tenth of the pre-activations exactly 0"
    # lr = 0: the weights stay integers through the call's three updates (an Adam step would move every weight by about lr, whatever its
    # gradient, and push the pre-activations off the kink by amounts that depend on rounding)
    l64, ea64, st64, _ = torch_reference(pkg, [model, None], [model, None], batch, 0.9, 0.0, torch.float64)
    _, ea32, _, _ = torch_reference(pkg, [model, None], [model, None], batch, 0.9, 0.0, torch.float32)
    losses, got = SpatialCall(pkg, env3, [model, None], [model, None], batch, 0.9, lr=0.0).step()
    assert got[0]["step"] == st64[0]
    compare_tensors(model, got[0]["exp_avg"], ea64[0], ea32[0], "integer convolutions")
    np.testing.assert_allclose(losses[0], l64[0][0], rtol=1e-4)


# ---- 3. step semantics ----------------------------------------------------------------------------------------------------------------------
def _small(pkg, Fn=2, seed=21):
    return [make_model(pkg, N5, C3, Fn, [3], [1], [1], 3, [1], 2, 7, [6], (5, 4)[t], seed + t) for t in range(2)]


def test_an_empty_list_takes_no_step(pkg, env3):
    """Agent 2 is never the imposter: the imposter team updates twice (agents 0 and 1), the crew team three times."""
    rng = np.random.default_rng(31)
    models = _small(pkg)
    batch = make_batch(rng, 20, 2, A3, C3, N5, 2, 4)
    batch["imposters"] = (np.arange(len(batch["imposters"])) % 2).astype(np.int16)
    l64, ea64, st64, _ = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float64)
    _, ea32, _, _ = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float32)
    losses, got = SpatialCall(pkg, env3, models, models, batch, 0.9).step()
    assert [got[0]["step"], got[1]["step"]] == st64 == [2.0, 3.0]
    for t in range(2):
        compare_tensors(models[t], got[t]["exp_avg"], ea64[t], ea32[t], f"team {t}")
    np.testing.assert_allclose(losses, l64[0], rtol=1e-4)


def test_done_rows_have_no_target_term(pkg, env3):
    """Every row is done: y = r, so the result does not depend on the target network at all -- bit for bit -- and matches float64."""
    rng = np.random.default_rng(32)
    models = _small(pkg)
    other = _small(pkg, seed=77)
    batch = make_batch(rng, 20, 2, A3, C3, N5, 2, 4)
    batch["dones"][:] = 1
    l64, _, _, _ = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float64)
    la, a = SpatialCall(pkg, env3, models, models, batch, 0.9).step()
    lb, b = SpatialCall(pkg, env3, models, other, batch, 0.9).step()
    np.testing.assert_allclose(la, l64[0], rtol=1e-4)
    assert np.array_equal(la, lb)
    for t in range(2):
        assert all(np.array_equal(x, y) for x, y in zip(a[t]["bits"], b[t]["bits"]))


def test_three_steps_match_the_float32_torch_path(pkg, env3):
    """Gradient accumulation over the agents and Adam's bias correction: three consecutive calls against three torch_train_step calls in
    float32 (test_gpu_train.py's tolerances: losses rtol 1e-4 / atol 1e-6, parameters rtol 1e-5 / atol 1e-6)."""
    rng = np.random.default_rng(33)
    models = _small(pkg)
    batch = make_batch(rng, 40, 2, A3, C3, N5, 2, 4)
    l32, _, st32, p32 = torch_reference(pkg, models, models, batch, 0.9, 1e-3, torch.float32, steps=3)
    call = SpatialCall(pkg, env3, models, models, batch, 0.9)
    for k in range(3):
        losses, got = call.step()
        np.testing.assert_allclose(losses, l32[k], rtol=1e-4, atol=1e-6)
    for t in range(2):
        assert got[t]["step"] == st32[t] == 9.0
        for (name, g_), (_, r_) in zip(split(models[t], got[t]["params"]), split(models[t], p32[t])):
            np.testing.assert_allclose(g_, r_, rtol=1e-5, atol=1e-6, err_msg=f"team {t} {name}")


def test_n_zero_is_a_no_op_that_zeroes_the_losses(pkg, env3):
    rng = np.random.default_rng(34)
    models = _small(pkg)
    batch = make_batch(rng, 4, 2, A3, C3, N5, 2, 4)
    for k in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "idx"):
        batch[k] = batch[k][:0]
    call = SpatialCall(pkg, env3, models, models, batch, 0.9)
    before = [flat(m) for m in models]
    losses, got = call.step()
    assert np.array_equal(losses, [0.0, 0.0])
    for t in range(2):
        assert got[t]["step"] == 0.0 and np.array_equal(got[t]["params"], before[t].astype(np.float32).astype(np.float64))
        assert not got[t]["exp_avg"].any() and not got[t]["exp_avg_sq"].any()


# ---- 4. the reference's own fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["global", "perspective"])
def test_reference_trainer_fixture(pkg, name):
    """The unmodified reference DQNTeamTrainer.train_step with SpatialDQN and the reference's featurizers on a reference ReplayBuffer
    (tests/golden/generate_train_spatial.py), through DeviceDQNTeamTrainer(spatial=True) on the fixture's ring -- the package's featurizer
    kernel included: losses at every step, the first step's gradients, the parameters after every step, the Adam step counts
    (spatial_train_fixtures.py has the criteria: those of the other learners' fixtures)."""
    from spatial_train_fixtures import TEAMS, check_step, load, models_from, step_indices

    meta, d = load(name)
    k = dict(meta["kwargs"])
    env = pkg.BatchedFourRoomEnv(k.pop("n_imposters"), k.pop("n_crew"), k.pop("n_jobs"), grid=np.array(meta["grid"], dtype=bool), **k, batch=64,
                                 device=DEV, rng="philox", seed=1, auto_reset=True)
    M = d["ring::states"].shape[0]
    ring = pkg.DeviceReplayBuffer(M, meta["state_size"], meta["T"], meta["n_agents"], meta["n_imposters"], device=DEV)
    for key in ("states", "next_states", "actions", "rewards", "dones", "imposters"):
        dst = getattr(ring, key)
        dst.copy_(torch.tensor(d["ring::" + key]).reshape(dst.shape).to(dst.dtype))
    ring.size = ring.idx = M
    models = [m.to(DEV) for m in models_from(pkg, meta, d)]
    fz = (pkg.GlobalFeaturizer if name == "global" else pkg.PerspectiveFeaturizer)(env)
    tr = pkg.DeviceDQNTeamTrainer(env, models[0], models[1], [], meta["lr"], meta["gamma"], featurizer=fz, spatial=True)
    assert tr.uses_spatial(ring)
    for step, idx in enumerate(step_indices(meta, d)):
        losses = tr.train_step_on_indices(ring, torch.tensor(idx, device=DEV)).cpu().numpy()
        print(f"step {step}: losses {losses} reference {d['losses'][step]}")
        np.testing.assert_allclose(losses, d["losses"][step], rtol=1e-4, atol=1e-6, err_msg=f"step {step}")
        ea = None
        if step == 0:
            ea = [dict((n, v) for (n, v) in split(models[t], tr.state_tensors(t)[0].cpu().numpy())) for t in range(2)]
        check_step(d, step, models, ea)
    for t, team in enumerate(TEAMS):
        assert float(tr.state_tensors(t)[2]) == meta["final_step"][team]


# ---- 5. reproducible, capturable, wired --------------------------------------------------------------------------------------------------
def test_two_runs_leave_identical_bytes(pkg, env3):
    rng = np.random.default_rng(51)
    n, T, Fn, imp, crew = RAGGED[3]
    models = _nets(pkg, Fn, (imp, crew), seed=3)
    batch = make_batch(rng, n, T, A3, C3, N5, Fn, 4)
    runs = []
    for _ in range(2):
        call = SpatialCall(pkg, env3, models, models, batch, 0.9)
        call.step()
        runs.append(call.step())
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))
    for t in range(2):
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(runs[0][1][t]["bits"], runs[1][1][t]["bits"]))


def test_graph_replay_matches_eager(pkg, env3):
    """A captured call replayed (single stream) equals the eager call."""
    rng = np.random.default_rng(52)
    models = _small(pkg)
    batch = make_batch(rng, 40, 2, A3, C3, N5, 2, 4)
    eager = SpatialCall(pkg, env3, models, models, batch, 0.9)
    want = [eager.step() for _ in range(3)]
    call = SpatialCall(pkg, env3, models, models, batch, 0.9)
    call.step()  # one eager step first: kernel attributes (step 1 of 3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    state = [g[k].buf for g in call.bufs for k in ("params", "exp_avg", "exp_avg_sq")] + [g["step"] for g in call.bufs]
    saved = [x.clone() for x in state]
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call.launch()
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip(state, saved):  # (capturing runs nothing; restore in case the runtime did)
        x.copy_(sv)
    for k in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        losses, got = call.results()
        assert np.array_equal(losses, want[k][0]), k
        for t in range(2):
            assert all(np.array_equal(x, y) for x, y in zip(got[t]["bits"], want[k][1][t]["bits"])), (k, t)


def _game_1v2(pkg, **kw):
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=5, auto_reset=True, grid_size=14, shuffle_imposter_index=True, **kw)


def _trainer_models(pkg, env, Fz, T_net=None):
    fz = Fz(env)
    _, planes, non = env._make_obs(fz.config, 1, rows=1)
    Fn = non.shape[-1] + (env.n_agents if Fz is pkg.GlobalFeaturizer else 0)
    C_, N_ = planes.shape[-3], planes.shape[-1]
    mk = lambda n_actions, seed: make_model(pkg, N_, C_, Fn, [4], [1], [1], 3, [1], 2, 16, [12], n_actions, seed)
    return mk(env.n_imposter_actions, 1), mk(env.n_crew_actions, 2)


def _same_adam_state(tr, twin, steps):
    for t in range(2):
        ea, _, step = tr.state_tensors(t)
        sd = twin.optimizer_state_dict(t)["state"]
        assert float(step) == steps == float(sd[0]["step"])
        want = torch.cat([sd[i]["exp_avg"].reshape(-1) for i in range(len(sd))]).cpu().numpy().astype(np.float64)
        compare_tensors(tr.models[t], ea.cpu().numpy().astype(np.float64), want, want, f"team {t} exp_avg")


@pytest.mark.parametrize("Fz", ["GlobalFeaturizer", "PerspectiveFeaturizer"])
def test_trainer_takes_the_path_and_matches_the_torch_path(pkg, Fz):
    """DeviceDQNTeamTrainer(spatial=True) on a real ring with T = 2: takes the path, and steps match a spatial=False twin (the torch path on
    the device, float32): losses rtol 1e-4 / atol 1e-6 at every step -- each depends on all the updates before it --, Adam's exp_avg per
    tensor within 1e-4 of its max-abs (the gradient criterion of the float64 tests), step counts exact.  Parameters are NOT compared
    element by element between the two float32 runs here: Adam moves a parameter by about lr whatever its gradient's size, so an element
    whose gradient is a near-cancelling sum differs by lr x (the relative rounding difference of that sum) per step -- measured: 1 of
    14116 elements 5.5e-6 apart after three steps of lr = 1e-3 (test_three_steps_match_the_float32_torch_path makes that comparison on
    a case where it holds, the float64 tests bound the gradients).  A SpatialQNet of the trained model sees the step without a refresh;
    switching to the torch step and back keeps the Adam state."""
    Fz = getattr(pkg, Fz)
    env = _game_1v2(pkg)
    ring = pkg.DeviceReplayBuffer(env.batch * 6, env.flattened_state_size, 2, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 6)
    imp, crew = _trainer_models(pkg, env, Fz)
    imp2, crew2 = copy.deepcopy(imp), copy.deepcopy(crew)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], 1e-3, 0.9, featurizer=Fz(env), spatial=True)
    twin = pkg.DeviceDQNTeamTrainer(env, imp2, crew2, [], 1e-3, 0.9, featurizer=Fz(env))
    assert tr.uses_spatial(ring) and not tr.hip and not tr.dense and not twin.uses_spatial(ring)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    idxs = [torch.randint(0, ring.size, (48,), device=DEV, generator=g) for _ in range(5)]
    for k in range(3):
        a, b = tr.train_step_on_indices(ring, idxs[k]), twin.train_step_on_indices(ring, idxs[k])
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    _same_adam_state(tr, twin, 9.0)
    # a SpatialQNet of the same model reads the parameters in place
    net = pkg.policy.SpatialQNet(env, imp)
    fz = Fz(env)
    fz.fit(ring.states[idxs[0]])
    roll = pkg.WindowedPolicyRollout.__new__(pkg.WindowedPolicyRollout)
    roll.env, roll.featurizer = env, fz
    sp, ns = roll.kernel_inputs()
    imp.eval()
    q = net.forward(sp, ns, agents=env.n_agents).clone()
    with torch.no_grad():
        want = torch.stack([imp(s, x) for s, x in fz.generate_featurized_states()], dim=1).reshape(-1, q.shape[-1])
    torch.testing.assert_close(q, want, rtol=1e-4, atol=1e-5)
    # the torch step, then the spatial step again: the Adam state travels
    tr.spatial = False
    a, b = tr.train_step_on_indices(ring, idxs[3]), twin.train_step_on_indices(ring, idxs[3])
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    tr.spatial = True
    a, b = tr.train_step_on_indices(ring, idxs[4]), twin.train_step_on_indices(ring, idxs[4])
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    _same_adam_state(tr, twin, 15.0)
    tr.sync_targets()
    assert all(torch.equal(tr.flat[t], tr.target_flat[t]) for t in range(2))


def test_spatial_is_opt_in(pkg):
    """spatial=False (the default) is the trainer as it was.  On the fused learner's layout (bitwise reproducible, so bits can be compared)
    a trainer built with spatial=False leaves the same bits as one built without the argument, and so does spatial=True: uses_hip goes first.
    A SpatialDQN without the flag takes the torch path (whose device kernels are not reproducible run to run: compared by tolerance)."""
    assert inspect.signature(pkg.DeviceDQNTeamTrainer.__init__).parameters["spatial"].default is False
    env = _game_1v2(pkg)
    ring = pkg.DeviceReplayBuffer(env.batch * 4, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 4)
    idx = torch.randint(0, ring.size, (32,), device=DEV)
    comps = ["onehot_pos", "alive_crew", "closest_crew"]
    out = []
    for kw in ({}, {"spatial": False}, {"spatial": True}):
        a, b = pkg.policy.reference_imposter_mlp(env, comps, seed=3), pkg.policy.reference_crew_mlp(env, comps, seed=4)
        tr = pkg.DeviceDQNTeamTrainer(env, a, b, comps, 1e-3, 0.9, **kw)
        assert tr.uses_hip(ring) and not tr.spatial and not tr.uses_spatial(ring)
        out.append((tr.train_step_on_indices(ring, idx), tr.flat[0].clone(), tr.flat[1].clone(), tr.exp_avg[0].clone(), tr.exp_avg_sq[1].clone()))
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(*out))
    imp, crew = _trainer_models(pkg, env, pkg.GlobalFeaturizer)
    out = []
    for kw in ({}, {"spatial": False}):
        a, b = copy.deepcopy(imp), copy.deepcopy(crew)
        tr = pkg.DeviceDQNTeamTrainer(env, a, b, [], 1e-3, 0.9, featurizer=pkg.GlobalFeaturizer(env), **kw)
        assert not tr.spatial and not tr.uses_spatial(ring) and not tr.hip
        out.append((tr.train_step_on_indices(ring, idx), tr.flat[0].clone(), tr.flat[1].clone()))
    for x, y in zip(*out):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-6)


def test_unserved_trainers_fall_back(pkg):
    """spatial=True where the step does not serve the trainer: uses_spatial is False and the torch path runs."""
    env = _game_1v2(pkg)
    ring = pkg.DeviceReplayBuffer(env.batch * 2, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 2)
    fz = pkg.GlobalFeaturizer(env)
    _, planes, non = env._make_obs(fz.config, 1, rows=1)
    Fn, C_, N_ = non.shape[-1] + env.n_agents, planes.shape[-3], planes.shape[-1]
    good = make_model(pkg, N_, C_, Fn, [], [1], [0], 3, [1], 1, 8, [8], env.n_imposter_actions, 1)
    assert pkg.DeviceDQNTeamTrainer(env, good, None, [], 1e-3, 0.9, featurizer=fz, spatial=True).uses_spatial(ring)
    dropout = make_model(pkg, N_, C_, Fn, [], [1], [0], 3, [1], 2, 8, [8], env.n_imposter_actions, 1, dropout=0.1)
    assert not pkg.DeviceDQNTeamTrainer(env, dropout, None, [], 1e-3, 0.9, featurizer=fz, spatial=True).uses_spatial(ring)
    flat_fz = pkg.FlatFeaturizer(env, ["onehot_pos"])
    assert not pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(good), None, ["onehot_pos"], 1e-3, 0.9, featurizer=flat_fz, spatial=True).uses_spatial(ring)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        oblong = pkg.SpatialDQN(N_, Fn, [C_], [1], [0], (3, 1), [1], 1, 8, 0.0, [8], env.n_imposter_actions)
    tr = pkg.DeviceDQNTeamTrainer(env, oblong, None, [], 1e-3, 0.9, featurizer=fz, spatial=True)
    assert not tr.uses_spatial(ring)
