"""The dense Q-network kernel (susnet_mlp_forward) and its wiring on the MI355X: exact against a float64 evaluation on integer-valued
networks at every ragged edge, close to the torch module on real observations, and -- through PolicyRollout / collect / train / evaluate --
bit-identical to the same calls made by hand on games no fused path serves."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")
CANARY = 12345.0


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def base_1v3(pkg, batch, seed=3, comps=COMPS3, **kw):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                  obs=pkg.ObsConfig("flat", comps), **kw)


def tagging_1v4(pkg, batch, seed=4, comps=("onehot_pos",), **kw):
    return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                             obs=pkg.ObsConfig("flat", list(comps)), **kw)


def seeded_mlp(pkg, dims, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = pkg.MLP(dims)
    return model.to(DEV).eval()


def mlp_forward(pkg, env, dims, weights, biases, slopes, rows, out):
    """susnet_mlp_forward by hand."""
    L = pkg._lib
    io = L.MlpIO()
    io.n_dims = len(dims)
    for k, d in enumerate(dims):
        io.dims[k] = d
    for l, (w, b) in enumerate(zip(weights, biases)):
        io.weight[l], io.bias[l] = w.data_ptr(), b.data_ptr()
    for l, s in enumerate(slopes):
        io.slope[l] = s.data_ptr()
    io.rows, io.n, io.q_out = rows.data_ptr(), rows.shape[0], out.data_ptr()
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_mlp_forward(env._h, C.byref(io), env._stream()))
    return out


def module_forward_by_hand(pkg, env, model, rows):
    lin, act = list(model.model)[0::2], list(model.model)[1::2]
    dims = [lin[0].in_features] + [m.out_features for m in lin]
    out = torch.empty(rows.shape[0], dims[-1], device=rows.device)
    return mlp_forward(pkg, env, dims, [m.weight for m in lin], [m.bias for m in lin], [m.weight for m in act], rows, out)


def tol(want):
    return 2e-5 * float(want.abs().max())  # the project's tolerance of its Q-network kernel against torch (test_gpu_parity.py)


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------------
EXACT_DIMS = [[36, 256, 128, 64, 16, 6], [88, 256, 128, 64, 16, 7], [37, 200, 100, 50, 16, 7], [4, 7], [1, 3, 2], [1024, 256, 32], [131, 33, 31, 5]]
EXACT_N = 320


def exact_network(dims, n, seed):
    """Weights / biases from {-1, 0, 1}, slopes 0.5, inputs from {0, 1} with a few 2 and 3; the float64 evaluation; and the precondition
    that makes float32 exact in any order: per layer max (sum |w||x| + |b|) * 2^(PReLUs passed) < 2^24 (a PReLU of slope 0.5 adds one
    binary place behind the point; every partial sum is a multiple of that place and below the bound)."""
    rng = np.random.default_rng(seed)
    W = [rng.choice([-1.0, 0.0, 1.0], size=(dims[l + 1], dims[l]), p=[0.3, 0.4, 0.3]) for l in range(len(dims) - 1)]
    Bv = [rng.choice([-1.0, 0.0, 1.0], size=dims[l + 1]) for l in range(len(dims) - 1)]
    x = rng.choice([0.0, 1.0], size=(n, dims[0]))
    x[rng.random(x.shape) < 0.02] = 2.0
    x[rng.random(x.shape) < 0.01] = 3.0
    h = x
    for l in range(len(W)):
        bound = float((np.abs(h) @ np.abs(W[l]).T + np.abs(Bv[l])).max()) * 2.0 ** l
        assert bound < 2.0 ** 24, (dims, l, bound)
        z = h @ W[l].T + Bv[l]
        h = np.where(z > 0, z, 0.5 * z) if l < len(W) - 1 else z
    want = h.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), h)
    return W, Bv, x, want


@pytest.fixture(scope="module")
def handle(pkg):
    env = base_1v3(pkg, 64)
    env.reset()
    return env


def to_device_at_odd_offsets(arrays):
    """Every array inside ONE float32 allocation, each starting 4 bytes past a 16-byte boundary or wherever the previous one ended plus one
    float: parameter tensors at arbitrary 4-byte offsets (a flat parameter buffer looks like this)."""
    total = sum(a.size + 1 for a in arrays) + 1
    flat = torch.full((total,), CANARY, dtype=torch.float32, device=DEV)
    views, off = [], 1
    for a in arrays:
        v = flat[off:off + a.size].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        views.append(v)
        off += a.size + 1
    return flat, views


def run_exact(pkg, env, dims, W, Bv, x, want, n):
    nl = len(W)
    _, views = to_device_at_odd_offsets(W + Bv + [np.full(1, 0.5)] * (nl - 1))
    Wd, Bd, Sd = views[:nl], views[nl:2 * nl], views[2 * nl:]
    F, n_out, pad_in, pad_out = dims[0], dims[-1], 3, 5
    inbuf = torch.full((n * F + 2 * pad_in,), CANARY, dtype=torch.float32, device=DEV)
    rows = inbuf[pad_in:pad_in + n * F].view(n, F)
    rows.copy_(torch.from_numpy(x[:n].astype(np.float32)))
    outbuf = torch.full((n * n_out + 2 * pad_out,), CANARY, dtype=torch.float32, device=DEV)
    out = outbuf[pad_out:pad_out + n * n_out].view(n, n_out)
    mlp_forward(pkg, env, dims, Wd, Bd, Sd, rows, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want[:n].view(np.int32)), (dims, n, float(np.abs(got - want[:n]).max()))
    for buf, pad in ((inbuf, pad_in), (outbuf, pad_out)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), (dims, n, "canary")
    assert torch.equal(rows.cpu(), torch.from_numpy(x[:n].astype(np.float32)))


@pytest.mark.parametrize("dims", EXACT_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_dense_forward_is_exact_on_integer_networks(pkg, handle, dims):
    W, Bv, x, want = exact_network(dims, EXACT_N, seed=11 + len(dims) + dims[0])
    for n in (1, 33, 95, EXACT_N):
        run_exact(pkg, handle, dims, W, Bv, x, want, n)


def test_dense_forward_is_exact_with_more_tiles_than_workgroups(pkg, handle):
    L = pkg._lib
    n = L.MLP_MAX_GRID * L.MLP_ROW_TILE * 2 + 95  # every workgroup walks at least two tiles, the last tile is ragged
    assert -(-n // L.MLP_ROW_TILE) > L.MLP_MAX_GRID
    dims = [5, 33, 3]
    W, Bv, x, want = exact_network(dims, n, seed=5)
    run_exact(pkg, handle, dims, W, Bv, x, want, n)


# ---- 2. close to torch on real observations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["base_1v3", "tagging_1v4"])
def test_dense_forward_matches_the_torch_module_on_real_observations(pkg, game):
    env = base_1v3(pkg, 320) if game == "base_1v3" else tagging_1v4(pkg, 320)
    comps = list(env.obs_config.components)
    env.reset()
    for _ in range(20):
        env.step(env.sample_actions())
    model = seeded_mlp(pkg, [env.obs.shape[-1], 256, 128, 64, 16, env.n_imposter_actions], seed=2)
    pol = pkg.PolicyRollout(env, model, None, components=comps, dense=True)
    assert pol.fused_imposter is None and pol.dense_imposter is not None, "no compiled-in layout here: the dense kernel serves the model"
    q, _ = pol.q_rows()
    with torch.no_grad():
        want = model(pol._spatial, env.obs)
    torch.testing.assert_close(q, want, rtol=0, atol=tol(want))
    off = pkg.PolicyRollout(env, model, None, components=comps, dense=False)
    assert off.dense_imposter is None and off.fused_imposter is None
    assert torch.equal(off.q_rows()[0], want)  # the torch module, as before


# ---- 3. dense against fused on a compiled-in layout --------------------------------------------------------------------------------------
def test_dense_forward_matches_the_fused_kernel_on_a_compiled_in_layout(pkg):
    env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=320, device=DEV, rng="philox", seed=5, auto_reset=True, grid_size=14,
                                 obs=pkg.ObsConfig("flat", COMPS3))
    env.reset()
    for _ in range(20):
        env.step(env.sample_actions())
    model = pkg.policy.reference_imposter_mlp(env, COMPS3, seed=1)
    pol = pkg.PolicyRollout(env, model, None, components=COMPS3, dense=True)
    assert pol.fused_imposter is not None and pol.dense_imposter is None and pol.one_kernel_tick, "the compiled-in layouts keep their kernels"
    want = env.qnet_forward(pol.fused_imposter)
    got = pkg.DenseQNet(env, model).forward(env.obs)
    torch.testing.assert_close(got, want, rtol=0, atol=tol(want))


# ---- 4. follows the weights without a refresh --------------------------------------------------------------------------------------------
def test_dense_path_follows_in_place_updates_and_re_pointed_parameters(pkg):
    env = base_1v3(pkg, 192)
    env.reset()
    for _ in range(5):
        env.step(env.sample_actions())
    model = seeded_mlp(pkg, [env.obs.shape[-1], 200, 100, 50, 16, env.n_imposter_actions], seed=8)
    pol = pkg.PolicyRollout(env, model, None, components=COMPS3, dense=True)
    assert pol.dense_imposter is not None

    def check(what):
        q, _ = pol.q_rows()
        with torch.no_grad():
            want = model(pol._spatial, env.obs)
        torch.testing.assert_close(q, want, rtol=0, atol=tol(want), msg=lambda m: f"{what}: {m}")
        return q.clone()

    q0 = check("initial weights")
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5).add_(0.01)
    q1 = check("after an in-place update")
    assert not torch.equal(q0, q1)
    old_ptrs = [p.data_ptr() for p in model.parameters()]
    flat = pkg.trainer._flatten_into(model, env.device)
    assert [p.data_ptr() for p in model.parameters()] != old_ptrs
    flat.mul_(1.5)
    q2 = check("after re-pointing the parameters into a flat buffer and updating that")
    assert not torch.equal(q1, q2)


# ---- 5. acting is bit-identical to the hand-wired tick -----------------------------------------------------------------------------------
def test_dense_tick_equals_the_hand_wired_tick(pkg):
    B, T = 192, 40
    ea, eb = (tagging_1v4(pkg, B, seed=9, max_time_steps=25) for _ in range(2))
    F = ea.obs.shape[-1]
    imp = seeded_mlp(pkg, [F, 256, 128, 64, 16, ea.n_imposter_actions], seed=1)
    crew = seeded_mlp(pkg, [F, 96, 33, ea.n_crew_actions], seed=2)
    assert max(ea.n_imposter_actions, ea.n_crew_actions) <= 16
    ea.reset()
    eb.reset()
    pol = pkg.PolicyRollout(ea, imp, crew, components=["onehot_pos"], epsilon=0.3, mask_dead=True, dense=True)
    assert pol.dense_imposter is not None and pol.dense_crew is not None and not pol.one_kernel_tick
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    ends = 0
    for tick in range(T):
        a1, r1, d1, t1 = pol.tick()
        q_imp = module_forward_by_hand(pkg, eb, imp, eb.obs)
        q_crew = module_forward_by_hand(pkg, eb, crew, eb.obs)
        _, r2, d2, t2, _, a2 = eb.policy_step(q_imp, q_crew, epsilon=0.3, mask_dead=True)
        assert torch.equal(a1, a2), tick
        assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(d1, d2) and torch.equal(t1, t2), tick
        ends += int(d1.sum()) + int(t1.sum())
    assert ends > 0
    assert torch.equal(ea.observe(raw8), eb.observe(raw8)) and torch.equal(ea.obs, eb.obs)


def test_captured_dense_tick_replays_like_the_eager_one(pkg):
    """PolicyRollout.capture() with both teams on the dense kernel: the replayed graph equals eager dense ticks on a twin env bit for bit
    (the launch path, its one-time LDS opt-in included, is capturable), and -- the documented behaviour of a captured graph -- a replay
    follows an IN-PLACE update of the weights, because the kernel reads them where the parameters live."""
    B, n = 192, 4
    ea, eb = (tagging_1v4(pkg, B, seed=17, max_time_steps=9, check_errors=False, export_state=False) for _ in range(2))
    F = ea.obs.shape[-1]
    imp = seeded_mlp(pkg, [F, 256, 128, 64, 16, ea.n_imposter_actions], seed=11)
    crew = seeded_mlp(pkg, [F, 96, 33, ea.n_crew_actions], seed=12)
    ea.reset()
    eb.reset()
    pa, pb = (pkg.PolicyRollout(e, imp, crew, components=["onehot_pos"], epsilon=0.3, mask_dead=True, dense=True) for e in (ea, eb))
    assert pa.dense_imposter is not None and pa.dense_crew is not None and not pa.one_kernel_tick
    graph, out = pa.capture(n, record=True)
    assert pa.captured_warmup_ticks == 2
    for _ in range(pa.captured_warmup_ticks):
        pb.tick()
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    ends = 0
    for rep in range(3):
        if rep == 2:  # in place: the parameters stay where the captured launches read them
            with torch.no_grad():
                for p in list(imp.parameters()) + list(crew.parameters()):
                    p.mul_(-0.5).add_(0.01)
        graph.replay()
        torch.cuda.synchronize()
        for k in range(n):
            obs = eb.obs.clone()
            a, r, d, t = pb.tick()
            assert torch.equal(out["obs_before"][k], obs), (rep, k)
            assert torch.equal(out["actions"][k], a), (rep, k)
            assert torch.equal(out["rewards"][k].view(torch.int32), r.view(torch.int32)), (rep, k)
            assert torch.equal(out["done"][k], d) and torch.equal(out["truncated"][k], t), (rep, k)
        ends += int(out["done"].sum()) + int(out["truncated"].sum())
        if rep == 1:
            before = out["actions"].clone()
    assert ends > 0 and not torch.equal(before, out["actions"])
    assert torch.equal(ea.observe(raw8), eb.observe(raw8)) and torch.equal(ea.obs, eb.obs)


# ---- 6. collect on a game without a fused path -------------------------------------------------------------------------------------------
def test_collect_on_a_game_without_a_fused_path(pkg):
    L = pkg._lib
    B, ticks, block, eps = 128, 24, 5, 0.2
    env, twin = (base_1v3(pkg, B, seed=21, max_time_steps=30) for _ in range(2))
    imp = seeded_mlp(pkg, [env.obs.shape[-1], 256, 128, 64, 16, env.n_imposter_actions], seed=6)
    rows = B * 16  # 24 ticks x B transitions: wraps once
    ring, ring2 = (pkg.DeviceReplayBuffer(rows, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device) for _ in range(2))
    env.reset()
    twin.reset()
    pol = pkg.PolicyRollout(env, imp, None, components=COMPS3, dense=True)
    assert pol.fused_imposter is None and pol.dense_imposter is not None
    assert ring.collect(env, pol, ticks, epsilon=eps, mask_dead=True, ticks_per_append=block) == ticks * B
    # the twin, tick by tick: flat observation, dense forward, susnet_policy_step into the feed; one susnet_ring_append per block
    window = twin.observe(pkg.ObsConfig("raw", dtype=torch.uint8)).unsqueeze(1).contiguous()
    feed = twin.alloc_feed(block)
    io = ring2._ring_io(twin, feed, window)
    done, appends = 0, 0
    while done < ticks:
        n = min(block, ticks - done)
        for t in range(n):
            twin.refresh_obs()
            q = module_forward_by_hand(pkg, twin, imp, twin.obs)
            twin.policy_tick_into(feed, t, q_imposter=q, epsilon=eps, mask_dead=True)
        io.n_ticks, io.idx = n, ring2.idx
        with torch.cuda.device(twin.device):
            L.check(twin.lib.susnet_ring_append(twin._h, C.byref(io), twin._stream()))
        ring2.idx = (ring2.idx + n * B) % rows
        ring2.size = min(ring2.size + n * B, rows)
        done += n
        appends += 1
    torch.cuda.synchronize()
    assert appends == 5 and (ring.idx, ring.size) == (ring2.idx, ring2.size) == ((ticks * B) % rows, rows)
    for f in RING_FIELDS:
        assert torch.equal(getattr(ring, f), getattr(ring2, f)), f"ring.{f}"
    # the run is not trivial: the agents moved and took several different actions (24 ticks from a reset stay below max_time_steps = 30, and a
    # freshly initialised imposter network seldom ends a game that early: episode ends are not required here, test 5 covers them)
    assert not torch.equal(ring.states, ring.next_states) and len(torch.unique(ring.actions)) > 2
    twin.refresh_obs()
    assert torch.equal(env.obs, twin.obs)  # collect leaves env.obs on the current state


# ---- 7. train() and evaluate() run where they refused ------------------------------------------------------------------------------------
def test_train_and_evaluate_on_a_game_without_a_fused_path(pkg, tmp_path):
    B, num_steps, k, batch_size = 64, 32, 4, 16
    env = tagging_1v4(pkg, B, seed=13, max_time_steps=20)
    comps = ["onehot_pos"]
    imp = seeded_mlp(pkg, [env.obs.shape[-1], 256, 128, 64, 16, env.n_imposter_actions], seed=3)
    policy = pkg.PolicyRollout(env, imp, None, components=comps, mask_dead=True, dense=True)
    trainer = pkg.DeviceDQNTeamTrainer(env, imp, None, comps, lr=1e-3, gamma=0.9, policy=policy)
    ring = pkg.DeviceReplayBuffer(B * num_steps, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    assert policy.dense_imposter is not None and not trainer.uses_hip(ring)
    before = [p.detach().clone() for p in imp.parameters()]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    metrics = pkg.EpisodicMetricHandler()
    pkg.train(env, metrics, num_steps, ring, policy, trainer, pkg.ExponentialSchedule(1.0, 0.05, 30), tmp_path / "run", train_step_interval=k,
              batch_size=batch_size, generator=gen)
    losses = metrics.metrics[pkg.SusMetrics.IMPOSTER_LOSS]
    assert len(losses) == sum(b.trains for b in pkg.plan_blocks(num_steps, k)) == 1 + (num_steps - 1) // k
    assert all(math.isfinite(v) for v in losses) and any(v > 0 for v in losses)
    assert metrics.metrics[pkg.SusMetrics.CREW_LOSS] == [0.0] * len(losses)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, imp.parameters()))
    q, _ = policy.q_rows()
    with torch.no_grad():
        want = imp(policy._spatial, env.obs)
    torch.testing.assert_close(q, want, rtol=0, atol=tol(want))
    assert (tmp_path / "run" / "imposter_mlp_100%.pt").exists()

    out = pkg.evaluate(env, imp, None, comps, n_ticks=48, block_ticks=16)
    assert out["episodes"] > 0 and out["ticks"] == 48
    undecided = 1.0 - out["imposter_win_rate"] - out["crew_win_rate"]
    assert 0.0 <= out["imposter_win_rate"] <= 1.0 and 0.0 <= out["crew_win_rate"] <= 1.0 and -1e-12 <= undecided <= 1.0
    assert out["truncation_rate"] >= undecided - 1e-12  # an episode nobody won ran into the step limit
    assert math.isclose(out["imposter_win_rate"] + out["crew_win_rate"] + undecided, 1.0)

    # what is still refused
    with pytest.raises(ValueError, match="reference MLPs"):
        rnd = pkg.RandomEquiprobable(env.n_imposter_actions)
        bad = pkg.PolicyRollout(env, rnd, None, components=comps)
        pkg.train(env, pkg.EpisodicMetricHandler(), 4, ring, bad, pkg.DeviceDQNTeamTrainer(env, rnd, None, comps, lr=1e-3, gamma=0.9, policy=bad),
                  pkg.ExponentialSchedule(1.0, 0.1, 10), tmp_path / "bad")
    with pytest.raises(ValueError, match="reference MLPs"):
        pkg.run_experiment(env, 4, pkg.RandomEquiprobable(env.n_imposter_actions), None, comps, experiment_base_dir=tmp_path)
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.run_experiment(env, 4, imp, None, comps, sequence_length=2, experiment_base_dir=tmp_path)


def test_collect_and_train_refuse_more_than_sixteen_actions(pkg, tmp_path):
    """susnet_policy_step takes at most 16 actions per team: an 11-agent tagging game keeps the act() + env.step fallback for acting, and
    collect / train say so instead of launching."""
    env = pkg.BatchedFourRoomEnvWithTagging(1, 10, 4, batch=64, device=DEV, rng="philox", seed=2, auto_reset=True, grid_size=14,
                                            obs=pkg.ObsConfig("flat", ["onehot_pos"]))
    assert env.n_imposter_actions > 16
    env.reset()
    imp = seeded_mlp(pkg, [env.obs.shape[-1], 32, env.n_imposter_actions], seed=1)
    pol = pkg.PolicyRollout(env, imp, None, components=["onehot_pos"], dense=True)
    assert pol.dense_imposter is not None
    ring = pkg.DeviceReplayBuffer(256, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    with pytest.raises(ValueError, match="16 actions"):
        ring.collect(env, pol, 2)
    with pytest.raises(ValueError, match="16 actions"):
        pkg.train(env, pkg.EpisodicMetricHandler(), 4, ring, pol, pkg.DeviceDQNTeamTrainer(env, imp, None, ["onehot_pos"], lr=1e-3, gamma=0.9, policy=pol),
                  pkg.ExponentialSchedule(1.0, 0.1, 10), tmp_path)
    a, rew, done, trunc = pol.tick()  # acting still works: the dense forward, then act() + env.step
    assert tuple(a.shape) == (64, env.n_agents) and int(a.max()) < env.n_imposter_actions
