"""ACTING under dropout between the SpatialDQN's RNN layers, on the MI355X: the acting mask (susnet_spatial_act_dropout_mask) as
include/susnet.h states it, susnet_spatial_forward_dropout against the float64 restatement of a training-mode forward GIVEN those masks
(spatial_dropout_util.masked_forward, pinned to the reference's module by test_spatial_dropout_host.py), exactly on integer networks, its
degenerate forms against susnet_spatial_forward bit for bit, its independence of tile and grid, and the path up: SpatialQNet,
WindowedPolicyRollout.q_rows, DeviceReplayBuffer.collect and run_experiment.

Shapes: 66 rows (22 envs x 3 agents: one full 64-row tile and a ragged one) and 1 row; H = 12 and 33 (below one 32-unit block, and one
unit into the second: 33 is no multiple of the four units of a Philox block); L = 2 (one buffer of products), 3 and 4 (two, alternating);
T = 1 .. 3; once the notebook's recurrence and head (H = 64, L = 3, T = 6, head [16, 16]); 16 448 and 32 865 rows of a tiny network: 257 full
tiles, and more tiles than the grid's 512 workgroups."""
import copy
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

from spatial_act_dropout_util import (SEED, export_act_mask, forward_net, header_act_mask, header_multiplier, layout_inputs, make_act_drop,
                                      masked_evaluate64)
from spatial_dropout_util import export_mask, make_drop, masked_forward
from spatial_exact import CANARY, exact_inputs, make_net, padded, to_device_at_odd_offsets, upload
from spatial_train_util import make_model

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
N5, C3, FN2, A3 = 5, 3, 2, 3
NINE = (9, 7, 3, [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], 8)  # test_gpu_spatial.py's whole-network stack


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env3(pkg):
    """The 3-agent 9 x 9 handle of the dropout tests: the network entry points take the error conventions from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. the acting mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_acting_mask_is_the_headers(pkg, env3, p):
    L = pkg._lib
    agents, layers, n, T, H = 3, 3, 7, 3, 33  # a ragged last env (7 = 2 x 3 + 1), a ragged last Philox block (33 = 8 x 4 + 1)
    get = lambda net=2, rows=n, **kw: export_act_mask(pkg, env3, make_act_drop(L, p, net, **dict(dict(offset=5), **kw)), net, agents, layers, rows, T, H)
    m = get()
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert m.dtype == np.float32 and np.isin(m, (np.float32(0.0), s)).all() and (m == 0).any() and (m == s).any()
    for net in (2, 3):  # element by element
        want = header_act_mask(p, SEED, 5, net, agents, 0, layers, n, T, H)
        assert np.array_equal(bits(get(net)), bits(want)), net
    assert np.array_equal(bits(m), bits(get())), "equal arguments, equal bytes"
    assert not np.array_equal(m, get(3)), "net 2 != net 3"
    # the train step's masks of the same seed and offset (nets 0 / 1) at equal other coordinates: agent a's rows G = 0, 1, 2
    for a in range(agents):
        mine = m[:, a::agents]
        for net in (0, 1):
            theirs = export_mask(pkg, env3, make_drop(L, p, p, seed=SEED, offset=5), net, a, layers, mine.shape[1], T, H)
            assert theirs.shape == mine.shape and not np.array_equal(theirs, mine), (a, net)
    # row_base shifts envs: env 1's rows under row_base 0 are env 0's under row_base 1
    assert np.array_equal(bits(get(row_base=1)[:, :agents]), bits(m[:, agents:2 * agents]))
    for what, other in (("seed", get(seed=SEED + 1)), ("offset", get(offset=6)), ("offset hi", get(offset=5 + (1 << 32))), ("row_base hi", get(row_base=1 << 32))):
        assert not np.array_equal(m, other), what
    hi = export_act_mask(pkg, env3, make_act_drop(L, p, 3, offset=(3 << 32) + 9, row_base=(1 << 33) + 4), 3, agents, layers, 5, T, H)
    assert hi[1, 4, 2, 32] == header_multiplier(p, SEED, (3 << 32) + 9, 3, 1, (1 << 33) + 5, 2, 1, 32)
    assert (export_act_mask(pkg, env3, make_act_drop(L, 0.0, 2), 2, agents, layers, n, T, H) == 1.0).all()  # p = 0 keeps everything: 1.0f


# ---- 2. the forward against float64 ---------------------------------------------------------------------------------------------------------
def tol(want):
    return 2e-5 * float(want.abs().max())  # the project's Q-network tolerance (test_gpu_spatial.py)


def module_forward(pkg, env, model, qnet, layout, B, A, T, p, net, offset, row_base, rng):
    """One SpatialQNet.forward of a training-mode module on inputs laid out as ``layout`` at odd 4-byte offsets, rnn_in and q_out between
    canaries -> (q float32 [n, n_out] on the host, float64 restatement under the exported masks, the unmasked float64 forward)."""
    rnn = model.rnn.model
    n, R = B * A, qnet.R
    x, ns, rows_x, rows_ns = layout_inputs(rng, layout, B, T, A, C3, N5, FN2)
    flat, (xd, nsd) = to_device_at_odd_offsets([x, ns])
    in_buf, rnn_in = padded((n, T, R), 7)
    q_buf, q = padded((n, qnet.dims[-1]), 5)
    qnet._rnn_in = rnn_in  # (the workspace the object would make for itself, here between canaries)
    before = flat.clone()
    got = qnet.forward(xd, nsd, A, out=q, net=net, offset=offset, row_base=row_base)
    torch.cuda.synchronize()
    assert got.data_ptr() == q.data_ptr() and qnet._rnn_in.data_ptr() == rnn_in.data_ptr()
    for buf, pad in ((in_buf, 7), (q_buf, 5)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), "canary"
    assert torch.equal(before, flat), "inputs changed"
    drop = make_act_drop(pkg._lib, p, net, offset=offset, row_base=row_base)
    masks = [torch.as_tensor(m).double() for m in export_act_mask(pkg, env, drop, net, A, rnn.num_layers, n, T, rnn.hidden_size)]
    m64 = copy.deepcopy(model).cpu().double()
    with torch.no_grad():
        want = masked_forward(m64, torch.as_tensor(rows_x).double(), torch.as_tensor(rows_ns).double(), masks)
        plain = masked_forward(m64, torch.as_tensor(rows_x).double(), torch.as_tensor(rows_ns).double(), None)
    return q.cpu().double(), want, plain


@pytest.mark.parametrize("layers,hidden", [(2, 12), (2, 33), (3, 12), (3, 33), (4, 12), (4, 33)])
def test_forward_against_float64(pkg, env3, layers, hidden):
    """Per (L, H): T = 1, 2, 3 x p = 0.2, 0.5 x Global / Perspective on 66 rows, and the single row at T = 3.  Measured on the MI355X: see
    DESIGN.md section 7a (the printed maxima)."""
    rng = np.random.default_rng(100 * layers + hidden)
    worst = 0.0
    for p in (0.2, 0.5):
        model = make_model(pkg, N5, C3, FN2, [3], [1], [1], 3, [1], layers, hidden, [6], 5, seed=layers + hidden, dropout=p).to(DEV)
        assert model.training
        qnet = pkg.SpatialQNet(env3, model, act_dropout_seed=SEED)
        for T in (1, 2, 3):
            for layout in ("global", "perspective"):
                for B, A in ((22, 3),) + (((1, 1),) if T == 3 else ()):
                    net = 2 + (T + (layout == "global")) % 2
                    got, want, plain = module_forward(pkg, env3, model, qnet, layout, B, A, T, p, net, offset=T, row_base=5, rng=rng)
                    err, scale = float((got - want).abs().max()), float(want.abs().max())
                    print(f"L={layers} H={hidden} T={T} p={p} {layout} n={B * A} net={net}: max|err| = {err:.3e} = {err / scale:.3e} max|want|")
                    worst = max(worst, err / scale)
                    if B > 1:
                        assert float((plain - want).abs().max()) > 1e-3 * scale, "the masks must matter for the comparison to say anything"
                    assert err <= tol(want), (T, p, layout, B * A, err, tol(want))
    print(f"L={layers} H={hidden}: worst relative error {worst:.3e} of the allowed 2e-5")


def test_forward_against_float64_on_the_notebooks_recurrence(pkg, env3):
    """H = 64 (two 32-unit blocks), L = 3, T = 6, head [16, 16], p = 0.2: notebooks/experiment.ipynb's recurrence and head."""
    rng = np.random.default_rng(64)
    model = make_model(pkg, N5, C3, FN2, [3], [1], [1], 3, [1], 3, 64, [16, 16], 5, seed=64, dropout=0.2).to(DEV)
    qnet = pkg.SpatialQNet(env3, model, act_dropout_seed=SEED)
    for layout, net in (("global", 2), ("perspective", 3)):
        got, want, plain = module_forward(pkg, env3, model, qnet, layout, 22, 3, 6, 0.2, net, offset=9, row_base=0, rng=rng)
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"notebook {layout} net={net}: max|err| = {err:.3e} = {err / scale:.3e} max|want|")
        assert float((plain - want).abs().max()) > 1e-3 * scale
        assert err <= tol(want)


# ---- 3. exact on integer networks -----------------------------------------------------------------------------------------------------------
def exact_case(pkg, env, net, n, T, pattern, rng, act_net, offset, row_base):
    dev = upload(net)
    inp = exact_inputs(net, n, T, pattern, rng)
    drop = make_act_drop(pkg._lib, 0.5, act_net, offset=offset, row_base=row_base)
    masks = export_act_mask(pkg, env, drop, act_net, inp["A"], net["L"], n, T, net["H"])
    assert np.isin(masks, (0.0, 2.0)).all()  # p = 0.5: the multiplier is exactly 2.0f
    want = masked_evaluate64(net, inp["rows_x"], inp["rows_ns"], masks)
    plain = masked_evaluate64(net, inp["rows_x"], inp["rows_ns"], np.ones_like(masks))
    got = forward_net(pkg, env, net, dev, inp, n, T, drop, act_net)
    assert np.array_equal(bits(got), bits(want)), (net["L"], net["H"], n, T, pattern, float(np.abs(got - want).max()))
    return want, plain


@pytest.mark.parametrize("L_,H,T,head", [(2, 33, 3, [7]), (3, 64, 2, [16, 16, 6]), (4, 33, 3, [7]), (3, 12, 1, [5])])
def test_exact_on_integer_networks(pkg, env3, L_, H, T, head):
    """Pre-activations are 0 or at least 32 in magnitude (inputs 0, +-1 and, behind a mask, +-2; weights and biases multiples of 32), so tanh is
    exactly 0 / +-1 and every sum is exact in float32 in any order: q_out is the float64 restatement bit for bit."""
    rng = np.random.default_rng(300 + 10 * L_ + T)
    net = make_net(rng, *NINE, L_, H, head)
    differ = False
    for n, pattern, act_net in ((66, "shared", 2), (66, "persp", 3), (1, "persp", 2)):
        want, plain = exact_case(pkg, env3, net, n, T, pattern, rng, act_net, offset=T, row_base=11)
        differ = differ or not np.array_equal(want, plain)
    assert differ, "the masks change the answer"


@pytest.mark.parametrize("n", [16448, 32865])
def test_exact_with_more_tiles_than_workgroups(pkg, env3, n):
    """A tiny network on many rows.  16 448 rows are 257 full tiles; the recurrence kernel's grid is MLP_MAX_GRID = 512 workgroups, so it is
    the 32 865 rows (10 955 envs x 3 agents: 514 tiles, the last one ragged) that make workgroups walk a second tile."""
    Lc = pkg._lib
    assert n % Lc.MLP_ROW_TILE == 0 or -(-n // Lc.MLP_ROW_TILE) > Lc.MLP_MAX_GRID
    rng = np.random.default_rng(8)
    net = make_net(rng, 3, 2, 3, [(3, 1, 1, 1)], 2, L=2, H=5, head=[3])
    want, plain = exact_case(pkg, env3, net, n, 2, "shared", rng, 2, offset=1, row_base=0)
    assert not np.array_equal(want, plain)


# ---- 4. the degenerate forms ----------------------------------------------------------------------------------------------------------------
def real_net(rng, L_, H, head=(7,)):
    return make_net(rng, *NINE, L_, H, list(head), real=True)


def test_degenerate_forms_are_the_plain_forward_bit_for_bit(pkg, env3):
    L = pkg._lib
    rng = np.random.default_rng(41)
    n, T = 66, 3
    net = real_net(rng, 3, 33)
    dev, inp = upload(net), exact_inputs(net, n, T, "shared", rng)
    plain = forward_net(pkg, env3, net, dev, inp, n, T)
    under = forward_net(pkg, env3, net, dev, inp, n, T, make_act_drop(L, 0.5, 2), 2)
    assert not np.array_equal(bits(plain), bits(under)), "p = 0.5 is another forward"
    for p in (0.0, 2.0 ** -33, 2.0 ** -40):  # floor(p 2^32) == 0
        for act_net in (2, 3):
            assert np.array_equal(bits(forward_net(pkg, env3, net, dev, inp, n, T, make_act_drop(L, p, act_net, offset=4), act_net)), bits(plain)), (p, act_net)
    one = real_net(rng, 1, 33)
    dev1, inp1 = upload(one), exact_inputs(one, n, T, "persp", rng)
    assert np.array_equal(bits(forward_net(pkg, env3, one, dev1, inp1, n, T, make_act_drop(L, 0.5, 2), 2)), bits(forward_net(pkg, env3, one, dev1, inp1, n, T)))
    # a seeded SpatialQNet on a model in eval(): the plain call
    model = make_model(pkg, N5, C3, FN2, [3], [1], [1], 3, [1], 3, 33, [6], 5, seed=2, dropout=0.5).to(DEV)
    x, ns, _, _ = layout_inputs(rng, "global", 22, T, A3, C3, N5, FN2)
    xd, nsd = torch.as_tensor(x, device=DEV), torch.as_tensor(ns, device=DEV)
    seeded, unseeded = pkg.SpatialQNet(env3, model, act_dropout_seed=SEED), pkg.SpatialQNet(env3, model)
    q_train = seeded.forward(xd, nsd, A3, net=2, offset=1).clone()
    with pytest.raises(RuntimeError, match="training mode"):
        unseeded.forward(xd, nsd, A3)
    model.eval()
    q_eval = seeded.forward(xd, nsd, A3, net=3, offset=2).clone()
    assert torch.equal(q_eval, unseeded.forward(xd, nsd, A3)) and not torch.equal(q_eval, q_train)


# ---- 5. independence and determinism ---------------------------------------------------------------------------------------------------------
def test_mask_depends_on_its_coordinates_and_on_nothing_else(pkg, env3):
    L = pkg._lib
    rng = np.random.default_rng(51)
    B, n, T = 22, 66, 3
    net = real_net(rng, 3, 33)
    dev, inp = upload(net), exact_inputs(net, n, T, "shared", rng)
    run = lambda act_net=2, sub=inp, rows=n, **kw: forward_net(pkg, env3, net, dev, sub, rows, T, make_act_drop(L, 0.2, act_net, **dict(dict(offset=3), **kw)), act_net)
    a = run()
    assert np.array_equal(bits(a), bits(run())), "equal (inputs, seed, offset): equal bytes"
    for what, other in (("offset", run(offset=4)), ("seed", run(seed=SEED + 1)), ("net", run(3)), ("row_base", run(row_base=1))):
        changed = int((bits(a) != bits(other)).any(axis=1).sum())
        assert changed > n // 2, (what, changed)  # (seed 1: a statement about these masks, not a retry)
    # envs [k, k + m) forwarded alone with row_base = k: those rows' bytes -- the mask knows nothing of tile, wave or grid
    for k, m in ((0, 5), (7, 5), (21, 1)):
        sub = dict(inp, x=inp["x"][k:k + m], ns=inp["ns"][k:k + m], sp_shape=(m,) + tuple(inp["sp_shape"][1:]), ns_shape=(m,) + tuple(inp["ns_shape"][1:]))
        alone = run(sub=sub, rows=m * A3, row_base=k)
        assert np.array_equal(bits(alone), bits(a[k * A3:(k + m) * A3])), k
        if k:
            assert not np.array_equal(bits(run(sub=sub, rows=m * A3, row_base=0)), bits(alone))


# ---- 6. the policy ---------------------------------------------------------------------------------------------------------------------------
def raw_env(pkg, batch, seed):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                  obs=pkg.ObsConfig("raw", dtype=torch.uint8), max_time_steps=6)


def notebook_like(pkg, env, seeds=(3, 4), hidden=12):
    """The notebook's architecture at small widths on the Global featurizer's tensors of ``env``: rnn_layers 3, rnn_dropout 0.2; fresh
    modules, so in training mode."""
    _, planes, non = env._make_obs(pkg.ObsConfig("planes"), 1, rows=1)
    cfg = dict(input_image_size=planes.shape[-1], non_spatial_input_size=non.shape[-1] + env.n_agents, n_channels=[planes.shape[-3], 5, 3],
               strides=[1, 1], paddings=[1, 1], kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=hidden, rnn_dropout=0.2,
               mlp_hidden_layer_dims=[8, 8])
    out = []
    for seed, n in zip(seeds, (env.n_imposter_actions, env.n_crew_actions)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            out.append(pkg.SpatialDQN(**cfg, n_actions=n).to(DEV))
    return out


def test_q_rows_is_the_dropout_forward_at_act_ticks(pkg):
    env = raw_env(pkg, 64, seed=21)
    imp, crew = notebook_like(pkg, env)
    A, T, s = env.n_agents, 2, 17
    policy = pkg.WindowedPolicyRollout(env, pkg.GlobalFeaturizer(env), imp, crew, sequence_length=T, kernels=True, act_dropout_seed=s)
    assert policy.act_ticks == 0 and policy.spatial_imposter.act_dropout_seed == s == policy.spatial_crew.act_dropout_seed
    hand = [pkg.SpatialQNet(env, imp, act_dropout_seed=s), pkg.SpatialQNet(env, crew, act_dropout_seed=s)]
    env.reset()
    policy.reset_window()
    feed = env.alloc_feed(1)
    for tick in range(4):
        if tick == 2:
            crew.eval()  # one team under dropout is enough for the tick to use up its offset
        q_imp, q_crew = policy.q_rows()
        assert policy.act_ticks == tick + 1
        f = policy._feed
        want_imp = hand[0].forward(f.spatial, f.non_spatial, A, net=2, offset=tick)
        want_crew = hand[1].forward(f.spatial, f.non_spatial, A, net=3, offset=tick)
        assert torch.equal(q_imp, want_imp) and torch.equal(q_crew, want_crew), tick
        assert not torch.equal(q_imp, hand[0].forward(f.spatial, f.non_spatial, A, net=2, offset=tick + 1))
        assert not torch.equal(q_imp, hand[0].forward(f.spatial, f.non_spatial, A, net=3, offset=tick))
        env.agent_policy_tick_into(feed, 0, q_imp, q_crew, epsilon=0.0, mask_dead=True)
        policy.push(feed["done"][0], feed["truncated"][0], feed["obs"][0])
    # both teams in eval(): the plain forward, and no offset is used up
    imp.eval()
    q_imp, _ = policy.q_rows()
    assert policy.act_ticks == 4 and torch.equal(q_imp, pkg.SpatialQNet(env, imp).forward(policy._feed.spatial, policy._feed.non_spatial, A))
    # act() / step() go through the same forwards
    imp.train()
    runner = pkg.WindowedPolicyRollout(env, pkg.GlobalFeaturizer(env), imp, crew, sequence_length=T, kernels=True, act_dropout_seed=s, mask_dead=False)
    runner.reset()
    runner.featurizer.fit(runner.window)
    spatial, non_spatial = runner.kernel_inputs()
    greedy = [h.forward(spatial, non_spatial, A, net=2 + k, offset=0).argmax(1).view(env.batch, A) for k, h in enumerate(hand)]
    acted = runner.act().clone()
    assert torch.equal(acted, torch.where(env.imposter_mask, greedy[0], greedy[1])) and runner.act_ticks == 1
    # a refused call uses up no offset
    policy.act_ticks = 1 << 56
    with pytest.raises(pkg._lib.SusnetError, match="offset"):
        policy.q_rows()
    assert policy.act_ticks == 1 << 56


def test_collect_consumes_one_offset_per_tick(pkg):
    """6 ticks at epsilon 0, T = 2, B = 64, a random crew on the philox stream: the ring bytes of collect equal those of the same ticks
    driven by hand -- push, featurize, the forward under dropout at offsets 0 .. 5 as net 2, agent_policy_tick_into, one ring append."""
    L = pkg._lib
    B, T, ticks, s = 64, 2, 6, 23
    rings, policies = [], []
    for by_hand in (False, True):
        env = raw_env(pkg, B, seed=31)
        imp, _ = notebook_like(pkg, env)
        feat = pkg.GlobalFeaturizer(env)
        ring = pkg.DeviceReplayBuffer(B * ticks, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
        env.reset()
        if not by_hand:
            policy = pkg.WindowedPolicyRollout(env, feat, imp, None, sequence_length=T, kernels=True, act_dropout_seed=s)
            assert ring.collect(env, policy, ticks, epsilon=0.0, mask_dead=True, ticks_per_append=ticks) == ticks * B
            assert policy.act_ticks == ticks
            policies.append(policy)
        else:
            window = pkg.WindowedPolicyRollout(env, feat, imp, None, sequence_length=T, kernels=True)  # (its window and push only)
            qnet = pkg.SpatialQNet(env, imp, act_dropout_seed=s)
            first = env.observe(pkg.ObsConfig("raw", dtype=torch.uint8))
            carried = first.unsqueeze(1).repeat(1, T, 1).contiguous()
            window.load_window(carried)
            block = env.alloc_feed(ticks)
            sfeed = pkg.policy.SpatialFeed(env, feat, B, T)
            for k in range(ticks):
                if k:
                    window.push(block["done"][k - 1], block["truncated"][k - 1], block["obs"][k - 1])
                with torch.cuda.device(env.device):
                    sfeed.featurize(window.window)
                sfeed.finish()
                q = qnet.forward(sfeed.spatial, sfeed.non_spatial, env.n_agents, net=2, offset=k)
                env.agent_policy_tick_into(block, k, q, None, epsilon=0.0, mask_dead=True)
            io = ring._ring_io(env, block, carried)
            io.n_ticks, io.idx = ticks, 0
            with torch.cuda.device(env.device):
                L.check(env.lib.susnet_ring_append(env._h, C.byref(io), env._stream()))
        torch.cuda.synchronize()
        rings.append({f: getattr(ring, f).cpu().numpy().copy() for f in ("states", "actions", "rewards", "next_states", "dones", "imposters")})
    for f, a in rings[0].items():
        assert np.array_equal(a.view(np.uint8), rings[1][f].view(np.uint8)), f
    assert len(np.unique(rings[0]["actions"])) > 2
    # a second collect goes on at offset 6
    env = policies[0].env
    ring = pkg.DeviceReplayBuffer(B * 2, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
    ring.collect(env, policies[0], 2, epsilon=0.0)
    assert policies[0].act_ticks == ticks + 2


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------
def same_checkpoint(a, b):
    """Two loaded checkpoints, whatever their nesting: equal keys, tensors equal bit for bit, everything else equal."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_checkpoint(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_checkpoint(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, torch.nn.Module):
        return isinstance(b, torch.nn.Module) and same_checkpoint(a.state_dict(), b.state_dict())
    return a == b


def test_run_experiment_acts_and_trains_under_dropout(pkg, tmp_path):
    """run_experiment on base_1v3, 64 envs, T = 2, rnn_layers 3, rnn_dropout 0.2, models left in training mode as the reference's are:
    200 ticks, a train step every 5.  With both seeds the run acts (susnet_spatial_forward_dropout) and learns
    (susnet_spatial_train_step_dropout) under dropout, writes act_dropout_seed into config.json, and twice gives identical checkpoints;
    without act_dropout_seed the first acting forward refuses the training-mode models, as it does today."""
    num_steps = 200

    def run(base, **kw):
        env = raw_env(pkg, 64, seed=7)
        imp, crew = notebook_like(pkg, env)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5)
        pkg.run_experiment(env, num_steps=num_steps, imposter_model=imp, crew_model=crew, components=[], sequence_length=2, replay_buffer_size=4000,
                           replay_prepopulate_steps=4, batch_size=16, gamma=0.9, scheduler_time_steps=100, experiment_base_dir=base,
                           learning_rate=1e-3, train_step_interval=5, target_update_interval=50, num_checkpoint_saves=2,
                           featurizer=pkg.GlobalFeaturizer(env), generator=gen, **kw)
        torch.cuda.synchronize()
        (run_dir,) = list(base.iterdir())
        return imp, crew, json.loads((run_dir / "config.json").read_text()), run_dir

    imp, crew, config, run_dir = run(tmp_path / "a", rnn_dropout_seed=1, act_dropout_seed=2)
    assert imp.training and crew.training, "the models are left in the mode the caller gave them"
    assert config["act_dropout_seed"] == 2 and config["rnn_dropout_seed"] == 1 and config["train_step"] == "susnet_spatial_train_step"
    assert all(bool(torch.isfinite(p).all()) for m in (imp, crew) for p in m.parameters())
    imp2, crew2, _, run_dir2 = run(tmp_path / "b", rnn_dropout_seed=1, act_dropout_seed=2)
    names = sorted(p.name for p in run_dir.glob("*.pt"))
    assert names == sorted(p.name for p in run_dir2.glob("*.pt")) and "imposter_spatial_dqn_100%.pt" in names and "crew_spatial_dqn_100%.pt" in names
    for name in names:
        a, b = (torch.load(d / name, map_location="cpu", weights_only=False) for d in (run_dir, run_dir2))
        assert same_checkpoint(a, b), name
    for a, b in ((imp, imp2), (crew, crew2)):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    # another acting seed: other masks, other actions, other parameters
    imp3, _, config3, _ = run(tmp_path / "c", rnn_dropout_seed=1, act_dropout_seed=3)
    assert config3["act_dropout_seed"] == 3 and any(not torch.equal(p, q) for p, q in zip(imp.parameters(), imp3.parameters()))
    with pytest.raises(RuntimeError, match="training mode"):
        run(tmp_path / "d", rnn_dropout_seed=1)
    assert "act_dropout_seed" not in json.loads((next((tmp_path / "d").iterdir()) / "config.json").read_text())
