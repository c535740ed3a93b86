"""The SpatialDQN forward kernels (susnet_spatial_forward) and their wiring on the MI355X: the convolution stage and the whole network exact
against a float64 evaluation on integer-valued networks (tanh pinned to 0 / +-1 by pre-activations that are multiples of 32), close to the
reference's stored outputs and to the torch module on the fixtures, following parameter updates without a refresh, and -- through
WindowedPolicyRollout(kernels=True) -- acting as the same calls made by hand and as the torch modules wherever their Q gap decides.  The integer-valued networks, their
evaluation and the calls through the C ABI are tests/spatial_exact.py; test_gpu_spatial_limits.py goes on where this file stops."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from spatial_exact import DEV, make_net, run_exact, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def handle(pkg):
    env = pkg.BatchedFourRoomEnv(1, 3, 5, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9, obs=pkg.ObsConfig("flat", ["onehot_pos"]))
    env.reset()
    return env


def tol(want):
    return 2e-5 * float(want.abs().max())  # the project's Q-network tolerance (test_gpu_mlp_dense.py)


# ---- 1. the convolution stage, exact -------------------------------------------------------------------------------------------------------
# (N, C, k, [(out, stride, padding, dilation)], Fn): given straight through the C ABI
CONV_STACKS = {
    "9x9_c7_3x3_three": (9, 7, 3, [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], 20),
    "14x14_c10_s2p2d2": (14, 10, 3, [(12, 2, 2, 2), (12, 2, 2, 2)], 12),
    "9x9_5x5_p2": (9, 3, 5, [(6, 1, 2, 1)], 4),
    "1x1": (5, 4, 1, [(7, 1, 0, 1), (2, 1, 1, 1)], 3),
    "c18_to_32": (6, 18, 3, [(32, 1, 1, 1), (17, 2, 0, 1)], 0),
    "n1": (1, 3, 3, [(4, 1, 1, 1), (9, 1, 2, 2)], 1),
    "four_layers_s3": (16, 2, 3, [(4, 1, 0, 1), (8, 3, 1, 1), (16, 1, 1, 2), (3, 4, 3, 3)], 2),
}


@pytest.mark.parametrize("stack", list(CONV_STACKS))
def test_convolution_stage_is_exact_on_integer_networks(pkg, handle, stack):
    N, Cc, k, convs, Fn = CONV_STACKS[stack]
    rng = np.random.default_rng(sorted(CONV_STACKS).index(stack) + 100)
    net = make_net(rng, N, Cc, k, convs, Fn, L=1, H=16, head=[3])
    dev = upload(net)
    for n in (1, 33, 95, 320):
        for T in (1, 3):
            for pattern in ("shared", "persp"):
                run_exact(pkg, handle, net, dev, n, T, pattern, rng)


# ---- 2. the whole network, exact -----------------------------------------------------------------------------------------------------------
# (T, rnn layers, hidden, head, variant)
WHOLE = {
    "t1_l1_h16": (1, 1, 16, [6], None),
    "t2_l3_h64": (2, 3, 64, [16, 16, 6], None),
    "t3_l1_h33": (3, 1, 33, [31, 5], None),
    "t8_l1_h256": (8, 1, 256, [256, 32], None),
    "t3_l3_h33": (3, 3, 33, [7], None),
    "t8_l4_h64": (8, 4, 64, [16, 7], None),
    "t3_l2_h16_no_recurrence": (3, 2, 16, [5], "no_recurrence"),
    "t3_l1_h16_carry": (3, 1, 16, [5], "carry"),
}


@pytest.mark.parametrize("case", list(WHOLE))
def test_whole_network_is_exact_on_integer_networks(pkg, handle, case):
    T, L, H, head, variant = WHOLE[case]
    rng = np.random.default_rng(sorted(WHOLE).index(case) + 200)
    net = make_net(rng, 9, 7, 3, [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], 8, L, H, head, variant)
    dev = upload(net)
    for n in (1, 33, 95, 320):
        want = run_exact(pkg, handle, net, dev, n, T, "persp" if n % 2 else "shared", rng)
    assert len(np.unique(want, axis=0)) > 3, "the rows differ: the answer depends on the input"


def test_exact_with_more_tiles_than_workgroups(pkg, handle):
    L = pkg._lib
    n = max(L.SPATIAL_CONV_MAX_GRID * L.SPATIAL_CONV_GROUP, L.MLP_MAX_GRID * L.MLP_ROW_TILE) * 2 + 95  # both kernels walk >= 2 tiles, ragged ends
    assert n % 3 == 0 and -(-n // L.MLP_ROW_TILE) > L.MLP_MAX_GRID and -(-n // L.SPATIAL_CONV_GROUP) > 2 * L.SPATIAL_CONV_MAX_GRID
    rng = np.random.default_rng(7)
    net = make_net(rng, 3, 2, 3, [(3, 1, 1, 1)], 2, L=1, H=5, head=[3])
    run_exact(pkg, handle, net, upload(net), n, 1, "shared", rng)


# ---- 3. the reference's stored outputs and the torch module -----------------------------------------------------------------------------
def fixture_models(pkg, name):
    if name == "model_spatialdqn":
        z = np.load(os.path.join(GOLDEN, "model_spatialdqn.npz"), allow_pickle=False)
        meta = json.loads(str(z["meta"]))
        m = pkg.SpatialDQN(**meta["config"])
        m.load_state_dict({k: torch.from_numpy(z["param::" + k]) for k in meta["keys"]})
        return [("model", m, torch.from_numpy(z["input0"]), torch.from_numpy(z["input1"]), 1, torch.from_numpy(z["output"]))]
    z = np.load(os.path.join(GOLDEN, "spatial", name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    spatial, non_spatial = torch.from_numpy(z["spatial"].astype(np.float32)), torch.from_numpy(z["non_spatial"])
    out = []
    for team in ("imposter", "crew"):
        m = pkg.SpatialDQN(**dict(meta["config"], n_actions=meta["n_actions"][team]))
        m.load_state_dict({k[len(team) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(team + "::")})
        want = torch.from_numpy(z["q_" + team])
        out.append((team, m, spatial, non_spatial, spatial.shape[2], want.reshape(-1, want.shape[-1])))
    return out


@pytest.mark.parametrize("name", ["model_spatialdqn", "base_1v4_global_t6", "base14_1v2_persp_t3"])
def test_forward_matches_the_reference_outputs_and_the_torch_module(pkg, handle, name):
    """Measured on the MI355X (max |error| / tolerance 2e-5 max|want|), kernel against the reference's stored outputs: DESIGN.md section 7 ("The SpatialDQN forward kernels") records the figures this test prints."""
    for team, model, spatial, non_spatial, agents, want in fixture_models(pkg, name):
        model = model.to(DEV).eval()
        spatial, non_spatial, want = spatial.to(DEV), non_spatial.to(DEV), want.to(DEV)
        net = pkg.SpatialQNet(handle, model)
        assert net is not None
        got = net.forward(spatial, non_spatial, agents)
        with torch.no_grad():
            if spatial.dim() == 6:
                module = torch.stack([model(spatial[:, :, i], non_spatial[:, :, i]) for i in range(agents)], dim=1).reshape(want.shape)
                f64 = model.double()
                exact = torch.stack([f64(spatial[:, :, i].double(), non_spatial[:, :, i].double()) for i in range(agents)], dim=1).reshape(want.shape)
            else:
                module = model(spatial, non_spatial)
                exact = model.double()(spatial.double(), non_spatial.double())
        err_ref, err_mod = float((got - want).abs().max()), float((got - module).abs().max())
        err_k64, err_m64 = float((got.double() - exact).abs().max()), float((module.double() - exact).abs().max())
        print(f"{name}/{team}: max|want| {float(want.abs().max()):.4f} tol {tol(want):.3e}; kernel vs reference {err_ref:.3e}, vs torch module {err_mod:.3e}, "
              f"vs float64 module {err_k64:.3e}; torch module vs float64 module {err_m64:.3e}")
        assert err_ref <= tol(want), f"{name}/{team}: kernel vs the reference's outputs: max error {err_ref:.3e} > {tol(want):.3e}"
        assert err_mod <= tol(module), f"{name}/{team}: kernel vs the torch module: max error {err_mod:.3e} > {tol(module):.3e}"


# ---- 4. parameters are followed without a refresh ----------------------------------------------------------------------------------------
def test_forward_follows_optimizer_steps_and_load_state_dict(pkg, handle):
    team, model, spatial, non_spatial, agents, _ = fixture_models(pkg, "base14_1v2_persp_t3")[0]
    model = model.to(DEV).eval()
    spatial, non_spatial = spatial.to(DEV), non_spatial.to(DEV)
    net = pkg.SpatialQNet(handle, model)

    def check(what):
        got = net.forward(spatial, non_spatial, agents).clone()
        with torch.no_grad():
            want = torch.stack([model(spatial[:, :, i], non_spatial[:, :, i]) for i in range(agents)], dim=1).reshape(got.shape)
        err = float((got - want).abs().max())
        assert err <= tol(want), f"{what}: max error {err:.3e} > {tol(want):.3e}"
        return got

    q0 = check("initial weights")
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for p in model.parameters():  # (gradients given directly: the step is what is under test, and the RNN's backward wants training mode)
        p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 0.5
    opt.step()
    q1 = check("after an in-place optimizer.step()")
    assert not torch.equal(q0, q1)
    other = fixture_models(pkg, "base14_1v2_persp_t3")[0][1].state_dict()
    model.load_state_dict({k: v * 0.5 + 0.01 for k, v in other.items()})
    q2 = check("after load_state_dict")
    assert not torch.equal(q1, q2)


# ---- 5. the acting loop ------------------------------------------------------------------------------------------------------------------
def seeded_spatial(pkg, env, feat, seed, n_actions, rnn_layers, hidden, head):
    A = env.n_agents
    _, planes, ns = env._make_obs(feat.config, 1, rows=1)
    Fn = ns.shape[-1] + (A if isinstance(feat, pkg.GlobalFeaturizer) else 0)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = pkg.SpatialDQN(input_image_size=env.n_rows, non_spatial_input_size=Fn, n_channels=[planes.shape[-3], 6, 8], strides=[1, 1], paddings=[1, 1],
                           kernel_size=[3, 3], dilations=[1, 1], rnn_layers=rnn_layers, rnn_hidden_dim=hidden, rnn_dropout=0.0,
                           mlp_hidden_layer_dims=head, n_actions=n_actions)
        with torch.no_grad():  # (a default initialisation answers nearly every state with the same action: weights x 3, no head biases -- on
            for name, p in m.named_parameters():  # the fixtures' inputs the argmax then spreads over the actions and no top-two gap is near 0)
                if "bias" in name and "prediction_head" in name:
                    p.zero_()
                elif p.dim() > 1:
                    p.mul_(3.0)
    return m.to(DEV).eval()


def acting_setup(pkg, game):
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    if game == "base14_persp_t3":
        env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=384, device=DEV, rng="philox", seed=13, auto_reset=True, grid_size=14, obs=raw8)
        feat, T, shape = pkg.PerspectiveFeaturizer(env), 3, (1, 16, [12])
    else:
        env = pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=256, device=DEV, rng="philox", seed=14, auto_reset=True, grid_size=9, obs=raw8)
        feat, T, shape = pkg.GlobalFeaturizer(env), 2, (3, 64, [16, 16])
    imp = seeded_spatial(pkg, env, feat, 5, env.n_imposter_actions, *shape)
    crew = seeded_spatial(pkg, env, feat, 6, env.n_crew_actions, *shape)
    return env, feat, T, imp, crew


def torch_greedy_and_gap(feat, imp_mask, imp, crew):
    greedy, decided = [], []
    for i, (sp, ns) in enumerate(feat.generate_featurized_states()):
        qs = [imp(sp, ns), crew(sp, ns)]
        g, ok = [], []
        for q in qs:
            top = q.topk(2, dim=1).values
            g.append(q.argmax(1))
            ok.append((top[:, 0] - top[:, 1]) > 2 * tol(q))
        greedy.append(torch.where(imp_mask[:, i], g[0], g[1]))
        decided.append(torch.where(imp_mask[:, i], ok[0], ok[1]))
    return torch.stack(greedy, 1), torch.stack(decided, 1)


@pytest.mark.parametrize("game", ["base14_persp_t3", "tagging_global_t2"])
def test_windowed_rollout_on_the_kernels_acts_as_by_hand_and_as_the_torch_modules(pkg, game):
    env, feat, T, imp, crew = acting_setup(pkg, game)
    runner = pkg.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, epsilon=0.0, mask_dead=False, kernels=True)
    assert isinstance(runner.spatial_imposter, pkg.SpatialQNet) and isinstance(runner.spatial_crew, pkg.SpatialQNet)
    off = pkg.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T)
    assert off.spatial_imposter is None and off.spatial_crew is None  # the default: the torch modules, as before
    hand = [pkg.SpatialQNet(env, imp), pkg.SpatialQNet(env, crew)]  # (their own buffers)
    runner.reset()
    A, B = env.n_agents, env.batch
    rows = skipped = ends = 0
    seen = set()
    with torch.no_grad():
        for tick in range(30):
            feat.fit(runner.window)
            imp_mask = env.imposter_mask.clone()
            spatial, non_spatial = runner.kernel_inputs()
            q = [net.forward(spatial, non_spatial, A).argmax(1).view(B, A) for net in hand]
            by_hand = torch.where(imp_mask, q[0], q[1])
            twin, decided = torch_greedy_and_gap(feat, imp_mask, imp, crew)
            a, rew, done, trunc = runner.step()
            assert torch.equal(a, by_hand), f"tick {tick}: the runner's actions are the kernel's argmax on its own window"
            assert torch.equal(a[decided], twin[decided]), f"tick {tick}: {int((a != twin)[decided].sum())} decided rows differ from the torch modules"
            rows += decided.numel()
            skipped += int((~decided).sum())
            ends += int(done.sum()) + int(trunc.sum())
            seen.update(torch.unique(a).tolist())
    assert skipped <= 0.01 * rows, f"{skipped} of {rows} rows had a top-two gap within twice the tolerance"
    assert len(seen) > 2, "the networks answer different states with different actions"


def test_windowed_rollout_keeps_the_torch_path_for_a_team_that_is_not_served(pkg):
    env, feat, T, imp, crew = acting_setup(pkg, "base14_persp_t3")
    crew.prediction_head[1] = nn.PReLU(12).to(DEV)  # per-channel slopes: not served
    runner = pkg.WindowedPolicyRollout(env, feat, imp, crew, sequence_length=T, epsilon=0.0, mask_dead=False, kernels=True)
    assert isinstance(runner.spatial_imposter, pkg.SpatialQNet) and runner.spatial_crew is None
    runner.reset()
    with torch.no_grad():
        for tick in range(5):
            feat.fit(runner.window)
            imp_mask = env.imposter_mask.clone()
            twin, decided = torch_greedy_and_gap(feat, imp_mask, imp, crew)
            a, *_ = runner.step()
            assert torch.equal(a[~imp_mask], twin[~imp_mask]), "the crew's actions are the torch module's, bit for bit"
            assert torch.equal(a[decided], twin[decided])
