"""State windows on the dense path (sequence_length T > 1) on the MI355X: the push kernel (susnet_window_push) bit for bit against its
torch restatement; PolicyRollout(dense=True, sequence_length=T) tick by tick against a raw window kept in torch by the reference's rules;
DeviceReplayBuffer.collect against a hand-driven twin and against the reference trainer's own rings (tests/golden/window/); the dense
train step on [n, T, S] windows against the same calls made by hand and against the torch path; run_experiment / evaluate end to end."""
import copy
import ctypes as C
import glob
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN_DIR, load_golden

import qnet_exact as X
from train_exact import BETAS, abi_step

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")
CANARY = 12345.0
WINDOW_DIR = os.path.join(GOLDEN_DIR, "window")
WCOLLECT = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WINDOW_DIR, "wcollect_*.npz")))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


def base_1v3(pkg, batch, seed=3, comps=COMPS3, **kw):
    return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                  obs=pkg.ObsConfig("flat", comps), **kw)


def tagging_1v4(pkg, batch, seed=4, comps=("onehot_pos",), grid_size=9, **kw):
    return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=grid_size,
                                             obs=pkg.ObsConfig("flat", list(comps)), **kw)


def seeded_mlp(pkg, dims, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = pkg.MLP(dims)
    return model.to(DEV).eval()


def tol(want):
    return 2e-5 * float(want.abs().max())  # the project's tolerance of its Q-network kernels against torch (test_gpu_parity.py)


def module_forward_by_hand(pkg, env, model, rows):
    """susnet_mlp_forward by hand on ``rows``."""
    L = pkg._lib
    lin, act = list(model.model)[0::2], list(model.model)[1::2]
    dims = [lin[0].in_features] + [m.out_features for m in lin]
    out = torch.empty(rows.shape[0], dims[-1], device=rows.device)
    io = L.MlpIO()
    io.n_dims = len(dims)
    for k, d in enumerate(dims):
        io.dims[k] = d
    for l, m in enumerate(lin):
        io.weight[l], io.bias[l] = m.weight.data_ptr(), m.bias.data_ptr()
    for l, m in enumerate(act):
        io.slope[l] = m.weight.data_ptr()
    io.rows, io.n, io.q_out = rows.data_ptr(), rows.shape[0], out.data_ptr()
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_mlp_forward(env._h, C.byref(io), env._stream()))
    return out


def flat_window(pkg, env, comps, raw_window):
    """``susnet_featurize`` of a raw window ``[B, T, S]``: the feature window ``[B, T * F]``, oldest state first."""
    feats = env.featurize(raw_window, pkg.ObsConfig("flat", comps))
    return feats.reshape(feats.shape[0], -1).contiguous()


# ---- 1. the push kernel, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(pkg):
    env = base_1v3(pkg, 64)
    env.reset()
    return env


def push(pkg, env, fresh, src, dst, T, done=None, truncated=None):
    """susnet_window_push by hand."""
    L = pkg._lib
    io = L.WindowIO()
    io.fresh, io.src, io.dst = fresh.data_ptr(), src.data_ptr(), dst.data_ptr()
    io.done = done.data_ptr() if done is not None else None
    io.truncated = truncated.data_ptr() if truncated is not None else None
    io.T, io.F, io.n = T, fresh.shape[1], fresh.shape[0]
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_window_push(env._h, C.byref(io), env._stream()))
    return dst


def random_bits(gen, *shape):
    """Random 32-bit patterns as float32 (NaNs of many payloads, infinities and denormals among them), with -0.0 and two NaNs set by hand."""
    x = torch.randint(-2**31, 2**31, shape, dtype=torch.int64, device=DEV, generator=gen).to(torch.int32)
    flat = x.view(-1)
    flat[0] = -2**31                      # -0.0
    if flat.numel() > 2:
        flat[1], flat[2] = 0x7FC00001, -1  # a quiet NaN with a payload; a NaN of all ones
    return x.view(torch.float32)


def carved(n_floats, lead):
    """A contiguous float32 view of ``n_floats`` inside a canary-filled allocation, ``lead`` floats in (lead = 1: 4-byte aligned only)."""
    buf = torch.full((n_floats + lead + 3,), CANARY, dtype=torch.float32, device=DEV)
    view = buf[lead:lead + n_floats]
    assert view.data_ptr() % 16 == (4 * lead) % 16
    return buf, view


def flag_sets(gen, n):
    """name -> (done, truncated); uint8 / bool mixed, as the callers hand them in (a feed's bool slots, a step's bool outputs)."""
    rnd = lambda p: torch.rand(n, device=DEV, generator=gen) < p
    d, t = rnd(0.4), rnd(0.4)
    return {"both NULL": (None, None), "done only": (d.clone(), None), "truncated only": (None, t.to(torch.uint8)),
            "both, overlapping": (d | rnd(0.2), (d & rnd(0.5)) | t), "both, disjoint": (d.to(torch.uint8), t & ~d),
            "all ended": (torch.ones(n, dtype=torch.bool, device=DEV), rnd(0.5)),
            "none ended": (torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV))}


@pytest.mark.parametrize("T,F", [(1, 5), (2, 1), (2, 3), (3, 36), (2, 88), (8, 128), (4, 255)])
def test_push_kernel_bitwise(pkg, handle, T, F):
    """Every n x flag set of the shape: dst equals the torch restatement as int32, the canary floats around dst are untouched, src and
    fresh are unchanged.  dst sits 4 bytes past a 16-byte boundary (lead = 1) except for one 16-byte aligned case per shape."""
    ref = pkg.policy.window_push_reference
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 * T + F)
    W = T * F
    seen = set()
    for n in (1, 63, 64, 65, 257):
        fresh, src = random_bits(gen, n, F), random_bits(gen, n, W)
        fresh0, src0 = fresh.clone(), src.clone()
        for k, (name, (done, trunc)) in enumerate(flag_sets(gen, n).items()):
            lead = 4 if (n == 64 and k == 1) else 1
            buf, dst = carved(n * W, lead)
            dst = dst.view(n, W)
            push(pkg, handle, fresh, src, dst, T, done, trunc)
            want = ref(src0, fresh0, done, trunc)
            assert torch.equal(dst.view(torch.int32), want.view(torch.int32)), (n, name)
            assert bool((buf[:lead] == CANARY).all()) and bool((buf[lead + n * W:] == CANARY).all()), (n, name, "a canary was overwritten")
            assert torch.equal(src.view(torch.int32), src0.view(torch.int32)) and torch.equal(fresh.view(torch.int32), fresh0.view(torch.int32)), (n, name)
            ended = torch.zeros(n, dtype=torch.bool, device=DEV)
            for f in (done, trunc):
                ended |= f.bool() if f is not None else ended
            seen.add((bool(ended.any()), bool((~ended).any())))
    assert seen == {(True, True), (True, False), (False, True)}, "rows that ended and rows that went on, mixed and alone"


def test_push_ping_pong_and_adjacent_buffers(pkg, handle):
    """A -> B -> A: two pushes equal two restated steps.  A and B are the two halves of ONE allocation (B starts where A ends: disjoint
    ranges that touch are served)."""
    ref = pkg.policy.window_push_reference
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    n, T, F = 65, 3, 36
    both = torch.zeros(2, n, T * F, dtype=torch.float32, device=DEV)
    A, Bw = both[0], both[1]
    A.copy_(random_bits(gen, n, T * F))
    a0 = A.clone()
    f1, f2 = random_bits(gen, n, F), random_bits(gen, n, F)
    d1, t2 = torch.rand(n, device=DEV, generator=gen) < 0.3, torch.rand(n, device=DEV, generator=gen) < 0.3
    push(pkg, handle, f1, A, Bw, T, done=d1)
    w1 = ref(a0, f1, d1)
    assert torch.equal(Bw.view(torch.int32), w1.view(torch.int32)) and torch.equal(A.view(torch.int32), a0.view(torch.int32))
    push(pkg, handle, f2, Bw, A, T, truncated=t2)
    w2 = ref(w1, f2, None, t2)
    assert torch.equal(A.view(torch.int32), w2.view(torch.int32)) and torch.equal(Bw.view(torch.int32), w1.view(torch.int32))
    # T = 1: the window is the fresh row, whatever the flags say
    one = torch.empty(n, F, dtype=torch.float32, device=DEV)
    push(pkg, handle, f1, f2, one, 1, done=d1)
    assert torch.equal(one.view(torch.int32), f1.view(torch.int32))


# ---- 2. the windowed policy, tick by tick ------------------------------------------------------------------------------------------------
def oldest_segment_model(pkg, net, T, F):
    """An integer network of tests/qnet_exact.py over F inputs as ``MLP([T * F, ...])`` whose first layer reads the OLDEST state's
    columns only (zeros on the newer ones)."""
    W, b, slopes = net
    dims = [T * F] + [w.shape[0] for w in W]
    model = pkg.MLP(dims)
    lin, act = list(model.model)[0::2], list(model.model)[1::2]
    with torch.no_grad():
        for l, m in enumerate(lin):
            w = np.zeros((W[l].shape[0], dims[l]))
            w[:, :W[l].shape[1]] = W[l]
            m.weight.copy_(torch.from_numpy(w).float())
            m.bias.copy_(torch.from_numpy(b[l]).float())
        for m, s in zip(act, slopes):
            m.weight.fill_(s)
    return model.to(DEV).eval()


@pytest.mark.parametrize("T", [2, 3])
def test_windowed_policy_tick_by_tick(pkg, T):
    B, ticks = 128, 20
    env = base_1v3(pkg, B, seed=31, max_time_steps=6, check_errors=False)
    F = env.obs.shape[-1]
    imp = seeded_mlp(pkg, [T * F, 96, 33, env.n_imposter_actions], seed=5)
    crew = seeded_mlp(pkg, [T * F, 64, 32, 16, env.n_crew_actions], seed=6)
    env.reset()
    pol = pkg.PolicyRollout(env, imp, crew, components=COMPS3, epsilon=0.0, mask_dead=True, dense=True, sequence_length=T)
    assert pol.fused_imposter is None and pol.fused_crew is None and not pol.one_kernel_tick, "the compiled-in layouts read F inputs: never at T > 1"
    assert pol.dense_imposter.dims[0] == pol.dense_crew.dims[0] == T * F and pol.sequence_length == T
    # integer networks that read ONLY the oldest state of the window: their Q rows are exact, from the state T - 1 ticks back
    int_nets = [X.int_network([F, 33, 31, 17, 5, n_act], seed=70 + k, slopes=(0.5, 1.0, 0.25, 0.5)) for k, n_act in
                enumerate((env.n_imposter_actions, env.n_crew_actions))]
    probes = [pkg.policy.DenseQNet(env, oldest_segment_model(pkg, net, T, F)) for net in int_nets]
    assert all(p is not None for p in probes)
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    raw = env.observe(raw8).unsqueeze(1).repeat(1, T, 1)  # train.py:318-322
    assert torch.equal(pol.reset_window(), env.obs.repeat(1, T))
    ends, lagged, spatial = 0, 0, torch.zeros(B, 1, 1, device=DEV)
    for tick in range(ticks + 1):
        want_window = flat_window(pkg, env, COMPS3, raw)
        assert torch.equal(pol.window_feats.view(torch.int32), want_window.view(torch.int32)), f"window_feats before tick {tick}"
        q_imp, q_crew = pol.q_rows()
        with torch.no_grad():
            for got, model in ((q_imp, imp), (q_crew, crew)):
                want = model(spatial, want_window.view(B, T, F))  # MLP.forward flattens [B, T, F] (dqn.py:86-90)
                torch.testing.assert_close(got, want, rtol=0, atol=tol(want))
        oldest, newest = np_(want_window[:, :F]), np_(want_window[:, (T - 1) * F:])
        for probe, net in zip(probes, int_nets):
            want_q, _ = X.reference_q(net, oldest.astype(np.float64))
            X.assert_same_values(np_(probe.forward(pol.window_feats)), want_q, f"tick {tick}: Q from the oldest state of the window")
            lagged += int((want_q != X.reference_q(net, newest.astype(np.float64))[0]).any(axis=1).sum())
        if tick == ticks:
            break
        a, rew, done, trunc = pol.tick()
        ended = done | trunc
        ends += int(ended.sum())
        after = env.observe(raw8)  # (after the auto-reset where the episode ended)
        nxt = torch.roll(raw, shifts=-1, dims=1)  # train.py:388-389
        nxt[:, -1] = after
        raw = torch.where(ended.view(-1, 1, 1), after.unsqueeze(1).expand(-1, T, -1), nxt)  # train.py:441-445
    assert ends >= B, "every env ended at least one episode (max_time_steps = 6)"
    assert lagged > 0, "the window matters: somewhere the oldest state gives another Q row than the newest"
    # env.reset(): the window restarts from the fresh state by itself
    env.reset()
    pol.q_rows()
    assert torch.equal(pol.window_feats, env.obs.repeat(1, T))


# ---- 3. collect at T = 2 against a hand-driven twin --------------------------------------------------------------------------------------
def test_collect_windows_against_a_hand_driven_twin(pkg):
    L = pkg._lib
    ref = pkg.policy.window_push_reference
    B, T, ticks, block, eps = 128, 2, 24, 5, 0.2
    env, twin, env2 = (base_1v3(pkg, B, seed=21, max_time_steps=6, check_errors=False) for _ in range(3))
    F = env.obs.shape[-1]
    imp = seeded_mlp(pkg, [T * F, 128, 64, 16, env.n_imposter_actions], seed=6)
    rows = B * 16  # 24 ticks x B transitions: wraps once
    ring, ring_twin, ring2 = (pkg.DeviceReplayBuffer(rows, env.flattened_state_size, T, env.n_agents, env.n_imposters, device=env.device)
                              for _ in range(3))
    for e in (env, twin, env2):
        e.reset()
    pol = pkg.PolicyRollout(env, imp, None, components=COMPS3, dense=True, sequence_length=T)
    assert pol.fused_imposter is None and pol.dense_imposter is not None
    assert ring.collect(env, pol, ticks, epsilon=eps, mask_dead=True, ticks_per_append=block) == ticks * B
    # the twin, tick by tick: flat observation, the feature window by the torch restatement, the dense forward by hand, susnet_policy_step
    # into the feed; one susnet_ring_append per block
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    window = twin.observe(raw8).unsqueeze(1).repeat(1, T, 1).contiguous()
    feed = twin.alloc_feed(block)
    io = ring_twin._ring_io(twin, feed, window)
    feats = flat_window(pkg, twin, COMPS3, window)
    done_ticks, ends, last = 0, 0, None
    while done_ticks < ticks:
        n = min(block, ticks - done_ticks)
        for t in range(n):
            twin.refresh_obs()
            if last is not None:
                feats = ref(feats, twin.obs, feed["done"][last], feed["truncated"][last])
            q = module_forward_by_hand(pkg, twin, imp, feats)
            twin.policy_tick_into(feed, t, q_imposter=q, epsilon=eps, mask_dead=True)
            last = t
        ends += int((feed["done"][:n] | feed["truncated"][:n]).sum())
        io.n_ticks, io.idx = n, ring_twin.idx
        with torch.cuda.device(twin.device):
            L.check(twin.lib.susnet_ring_append(twin._h, C.byref(io), twin._stream()))
        ring_twin.idx = (ring_twin.idx + n * B) % rows
        ring_twin.size = min(ring_twin.size + n * B, rows)
        done_ticks += n
    torch.cuda.synchronize()
    assert ends > 0 and (ring.idx, ring.size) == (ring_twin.idx, ring_twin.size) == ((ticks * B) % rows, rows)
    for f in RING_FIELDS:
        assert torch.equal(getattr(ring, f), getattr(ring_twin, f)), f"ring.{f}"
    assert not torch.equal(ring.states[:, 0], ring.states[:, 1]) and len(torch.unique(ring.actions)) > 2
    twin.refresh_obs()
    assert torch.equal(env.obs, twin.obs)  # collect leaves env.obs on the current state
    # two calls (9 + 15 ticks) give the ring of one call: raw window and feature window carry over
    pol2 = pkg.PolicyRollout(env2, imp, None, components=COMPS3, dense=True, sequence_length=T)
    for part in (9, 15):
        assert ring2.collect(env2, pol2, part, epsilon=eps, mask_dead=True, ticks_per_append=block) == part * B
    assert (ring2.idx, ring2.size) == (ring.idx, ring.size)
    for f in RING_FIELDS:
        assert torch.equal(getattr(ring2, f), getattr(ring, f)), f"two calls: ring.{f}"
    # after env.reset() the window restarts from the fresh state: the next rows' T states are all the fresh one, and so is the feature window
    env.reset()
    fresh = env.observe(raw8).float()
    at = ring.idx
    assert ring.collect(env, pol, 1, epsilon=eps, mask_dead=True) == B
    new_rows = ring.states[at:at + B]
    assert torch.equal(new_rows[:, 0], fresh) and torch.equal(new_rows[:, 1], fresh)
    assert torch.equal(pol.window_feats, flat_window(pkg, env, COMPS3, new_rows))
    # a policy of another window length is refused
    with pytest.raises(AssertionError, match="trajectory_size"):
        pkg.DeviceReplayBuffer(rows, env.flattened_state_size, 3, env.n_agents, env.n_imposters, device=env.device).collect(env, pol, 1)


# ---- 4. the reference trainer's own rings at T = 2 and 3 ---------------------------------------------------------------------------------
def env_from_meta(pkg, meta, batch, **kw):
    k = dict(meta["kwargs"])
    k.pop("include_walls", None)
    grid = np.array(meta["grid_used"], dtype=bool)
    if meta["class"] == "itg":
        return pkg.BatchedImposterTrainingGround(**k, grid=grid, batch=batch, **kw)
    return pkg.BatchedFourRoomEnv(**k, grid=grid, batch=batch, **kw)


@pytest.mark.parametrize("name", WCOLLECT)
def test_windowed_collection_matches_the_reference_trainer_loop(pkg, name):
    """tests/golden/generate_collect_window.py: train.py:316-322, 345-399, 419-449 around the unmodified env, FlatFeaturizer, MLP([T F, ..])
    and ReplayBuffer; one env, numpy's words as the tape, the stored parameters, greedy."""
    g = load_golden(os.path.join(WINDOW_DIR, name + ".npz"))
    meta = g["meta"]
    T, max_size, num_steps, comps = meta["trajectory_size"], meta["max_size"], meta["num_steps"], meta["components"]
    assert T > 1
    env = env_from_meta(pkg, meta, 1, device=DEV, rng="numpy", tape_words=1 << 16, auto_reset=True, check_errors=False, obs=pkg.ObsConfig("flat", comps))
    env._reseed([meta["seed"]])
    models = []
    for team in ("imposter", "crew"):
        m = pkg.policy.MLP(meta[f"{team}_dims"])
        m.load_state_dict({k[len(team) + 2:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(team + "::")})
        models.append(m.to(DEV).eval())
    policy = pkg.PolicyRollout(env, *models, components=comps, mask_dead=True, dense=True, sequence_length=T)
    assert policy.dense_imposter is not None and policy.dense_crew is not None and policy.fused_imposter is None
    buf = pkg.DeviceReplayBuffer(max_size, meta["state_size"], T, meta["n_agents"], meta["n_imposters"], device=env.device)
    env.reset()
    for part in (37, num_steps - 37):  # two calls: the windows carry over
        assert buf.collect(env, policy, part, epsilon=0.0, mask_dead=True, ticks_per_append=50) == part
    torch.cuda.synchronize()
    env.poll_errors()
    assert (buf.idx, buf.size) == (meta["idx"], meta["size"])
    n = buf.size
    np.testing.assert_array_equal(np_(buf.actions[:n]), g["actions"].astype(np.int64), err_msg="actions (the networks' greedy choices)")
    np.testing.assert_array_equal(np_(buf.states[:n]), g["states"].astype(np.float32), err_msg="states")
    np.testing.assert_array_equal(np_(buf.next_states[:n]), g["next_states"].astype(np.float32), err_msg="next_states")
    assert np_(buf.rewards[:n]).view(np.uint32).tolist() == g["rewards"].view(np.uint32).tolist(), "rewards"
    np.testing.assert_array_equal(np_(buf.dones[:n]), g["dones"].astype(bool), err_msg="dones")
    np.testing.assert_array_equal(np_(buf.imposters[:n]), g["imposters"], err_msg="imposters")


# ---- 5. the dense train step on windows --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring_t2(pkg):
    """(env, ring): 9x9 1v3, populate_fused with batch 64 x 10 ticks at trajectory_size 2, some rows marked done (the ring is data)."""
    env = base_1v3(pkg, 64, seed=8, max_time_steps=7)
    ring = pkg.DeviceReplayBuffer(64 * 10, env.flattened_state_size, 2, env.n_agents, env.n_imposters, device=env.device)
    ring.populate_fused(env, 10)
    ring.dones[::3] = True
    torch.cuda.synchronize()
    return env, ring


def flat_params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("n", [1, 33])
def test_dense_train_step_on_windows(pkg, ring_t2, n):
    env, ring = ring_t2
    T, F = 2, env.obs.shape[-1]
    dims = ([T * F, 64, 33, env.n_imposter_actions], [T * F, 48, 16, 16, env.n_crew_actions])
    imp, crew = seeded_mlp(pkg, dims[0], seed=3), seeded_mlp(pkg, dims[1], seed=4)
    init = [flat_params(imp), flat_params(crew)]
    dense = pkg.DeviceDQNTeamTrainer(env, imp, crew, COMPS3, 1e-3, 0.9, dense=True)
    torch_tr = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(crew), COMPS3, 1e-3, 0.9)
    assert dense.uses_dense(ring) and not dense.uses_hip(ring) and dense.sequence_length == T
    assert not torch_tr.uses_dense(ring) and not torch_tr.uses_hip(ring)
    one_state = pkg.DeviceReplayBuffer(8, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    assert not dense.uses_dense(one_state), "these networks read two states"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(50 + n)
    idx = torch.randint(0, ring.size, (n,), device=DEV, generator=gen)
    if n > 1:
        idx[0], idx[1] = 0, 1  # a done row and one that is not
        assert bool(ring.dones[idx].any()) and not bool(ring.dones[idx].all())
    losses = dense.train_step_on_indices(ring, idx).clone()
    # by hand: gather, susnet_featurize over n * T rows ([n * T, F] is [n][T * F]), susnet_mlp_train_step
    oc = pkg.ObsConfig("flat", COMPS3)
    feat = env.featurize(ring.states[idx], oc).reshape(n, T * F)
    next_feat = env.featurize(ring.next_states[idx], oc).reshape(n, T * F)
    batch = dict(feat=np_(feat), next_feat=np_(next_feat), idx=np_(idx), actions=np_(ring.actions), rewards=np_(ring.rewards),
                 dones=np_(ring.dones).reshape(-1).astype(np.uint8), imposters=np_(ring.imposters).reshape(-1))
    teams = [dict(dims=d, params=init[t], target=init[t], lr=1e-3, betas=BETAS) for t, d in enumerate(dims)]
    hand_losses, hand = abi_step(pkg, env, teams, batch, 0.9)
    assert np_(losses).astype(np.float64).tolist() == hand_losses.tolist(), "losses"
    for t in range(2):
        ea, easq, step = dense.state_tensors(t)
        assert float(step) == hand[t]["step"] > 0
        assert np.array_equal(np_(dense.flat[t]).view(np.int32), hand[t]["params32"].view(np.int32)), f"team {t}: params"
        assert np.array_equal(np_(ea).astype(np.float64), hand[t]["exp_avg"]) and np.array_equal(np_(easq).astype(np.float64), hand[t]["exp_avg_sq"]), t
        assert not np.array_equal(np_(dense.flat[t]).astype(np.float64), init[t]), f"team {t} moved"
    # the torch path: torch_train_step through the package's FlatFeaturizer on the same [n, T, S] windows; the tolerances of
    # tests/test_gpu_mlp_train.py::_compare_two_steps (losses rtol 1e-4 / atol 1e-6, first-step exp_avg within 1e-4 of each tensor's max-abs)
    torch_losses = torch_tr.train_step_on_indices(ring, idx)
    torch.testing.assert_close(losses, torch_losses, rtol=1e-4, atol=1e-6)
    for t in range(2):
        ea, _, sa = dense.state_tensors(t)
        eb, _, sb = torch_tr.state_tensors(t)
        assert float(sa) == float(sb) > 0
        off = 0
        for name, p in dense.models[t].named_parameters():
            x, y = ea[off:off + p.numel()], eb[off:off + p.numel()]
            off += p.numel()
            assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-12, (t, name)


# ---- 6. run_experiment and evaluate ------------------------------------------------------------------------------------------------------
def test_run_experiment_and_evaluate_on_windows(pkg, tmp_path):
    B, num_steps, T, comps = 64, 32, 2, ["onehot_pos"]
    env = tagging_1v4(pkg, B, seed=13, max_time_steps=20)
    F = env.obs.shape[-1]
    imp = seeded_mlp(pkg, [T * F, 128, 64, 16, env.n_imposter_actions], seed=3)
    crew = seeded_mlp(pkg, [T * F, 64, 16, env.n_crew_actions], seed=4)
    before = [p.detach().clone() for m in (imp, crew) for p in m.parameters()]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    metrics = pkg.run_experiment(env, num_steps, imp, crew, comps, sequence_length=T, replay_buffer_size=B * 64, replay_prepopulate_steps=8,
                                 batch_size=16, gamma=0.9, scheduler_time_steps=30, experiment_base_dir=tmp_path / "exp", learning_rate=1e-3,
                                 train_step_interval=4, generator=gen)
    (run_dir,) = list((tmp_path / "exp").iterdir())
    assert json.loads((run_dir / "config.json").read_text())["sequence_length"] == 2
    for key in (pkg.SusMetrics.IMPOSTER_LOSS, pkg.SusMetrics.CREW_LOSS):
        losses = metrics.metrics[key]
        assert len(losses) == 1 + (num_steps - 1) // 4 and all(math.isfinite(v) for v in losses) and any(v > 0 for v in losses), key
    after = [p.detach() for m in (imp, crew) for p in m.parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    loaded = pkg.MLP.load_from_checkpoint(run_dir / "imposter_mlp_100%.pt", map_location="cpu")
    assert loaded.layer_dims == [T * F, 128, 64, 16, env.n_imposter_actions]
    assert all(torch.equal(a, b.detach().cpu()) for a, b in zip(loaded.parameters(), imp.parameters()))
    assert pkg.MLP.load_from_checkpoint(run_dir / "crew_mlp_100%.pt", map_location="cpu").layer_dims[0] == T * F

    out = pkg.evaluate(env, imp, crew, comps, n_ticks=48, block_ticks=16, sequence_length=T)
    assert out["episodes"] > 0 and out["ticks"] == 48
    for key in ("imposter_win_rate", "crew_win_rate", "truncation_rate"):
        assert 0.0 <= out[key] <= 1.0, key
    table = pkg.evaluate_checkpoints(run_dir, env, comps, n_ticks=24, block_ticks=8, sequence_length=T)
    assert "100%" in table and all(v["episodes"] > 0 for v in table.values())

    # what is refused: a network that reads ONE state, a window wider than the dense kernel's input, graph capture of windowed ticks
    one_state = seeded_mlp(pkg, [F, 64, env.n_imposter_actions], seed=5)
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.run_experiment(env, 4, one_state, None, comps, sequence_length=2, experiment_base_dir=tmp_path / "bad")
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.PolicyRollout(env, one_state, None, components=comps, dense=True, sequence_length=2)
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.PolicyRollout(env, imp, crew, components=comps, dense=False, sequence_length=2)
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.evaluate(env, one_state, None, comps, n_ticks=4, sequence_length=2)
    wide = tagging_1v4(pkg, 8, grid_size=14)
    F14 = wide.obs.shape[-1]
    assert 8 * F14 > pkg._lib.MLP_MAX_F >= 7 * F14
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.PolicyRollout(wide, pkg.MLP([8 * F14, 32, wide.n_imposter_actions]).to(DEV), None, components=comps, dense=True, sequence_length=8)
    pol = pkg.PolicyRollout(env, imp, crew, components=comps, dense=True, sequence_length=T)
    with pytest.raises(ValueError, match="sequence_length"):
        pol.capture(2)
