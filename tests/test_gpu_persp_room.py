"""The room-masked Perspective views on the MI355X: ``susnet_featurize`` in the modes SUSNET_OBS_PERSP_ROOM / _ROOM_MASK bit for bit against
the reference-pinned fixture and the host restatement (``features.room_mask_views``), windows, and the partially observable
``PerspectiveFeaturizer`` through acting, training, ``run_experiment`` and ``evaluate``."""
import copy
import ctypes as C
import importlib
import json
import math

import numpy as np
import pytest
import torch

import persp_room_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = (("persp_room", False), ("persp_room_mask", True))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


def raw8(pkg):
    return pkg.ObsConfig("raw", dtype=torch.uint8)


GAMES = {"base14_1v2_j4": ("base", 1, 2, 4, 14), "tagging_1v4_j5": ("tagging", 1, 4, 5, 9), "base_3v9_j4": ("base", 3, 9, 4, 9)}


def make_env(pkg, game, batch=8, **kw):
    kind, n_imp, n_crew, J, N = GAMES[game] if isinstance(game, str) else game
    cls = pkg.BatchedFourRoomEnvWithTagging if kind == "tagging" else pkg.BatchedFourRoomEnv
    return cls(n_imp, n_crew, J, batch=batch, device=DEV, rng="philox", seed=kw.pop("seed", 3), auto_reset=True, grid_size=N, obs=raw8(pkg), **kw)


@pytest.fixture(scope="module")
def envs(pkg):
    return {name: make_env(pkg, name) for name in GAMES}


# ---- 1. susnet_featurize, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_featurize_equals_the_reference_fixture(pkg, name):
    meta, d = U.load_fixture(name)
    k = meta["kwargs"]
    env = make_env(pkg, (meta["class"], k["n_imposters"], k["n_crew"], k["n_jobs"], 9))
    rows = torch.from_numpy(d["raw"]).to(DEV)
    for (mode, with_mask), dtype in ((m, t) for m in MODES for t in (torch.uint8, torch.float32)):
        sp, non = env.featurize(rows, pkg.ObsConfig(mode, dtype=dtype))
        assert sp.dtype == dtype and non.dtype == dtype
        np.testing.assert_array_equal(np_(sp), d["spatial_mask" if with_mask else "spatial"].astype(np_(sp).dtype), err_msg=f"{mode} {dtype}")
        np.testing.assert_array_equal(np_(non), d["non_spatial"].astype(np_(non).dtype), err_msg=f"{mode} {dtype} non-spatial")


@pytest.fixture(scope="module")
def restated(pkg, envs):
    """Per game: 129 random rows and their restated views (computed once; the tests take the first n rows)."""
    out = {}
    for seed, (name, env) in enumerate(envs.items()):
        kind, _, _, J, N = GAMES[name]
        rows = U.random_rows(np.random.default_rng(100 + seed), 129, env.n_agents, J, N, kind == "tagging")
        assert rows.shape[1] == env.flattened_state_size
        out[name] = (rows, pkg.features.room_mask_views(env, rows, True))
    return out


def featurize_at_offset(pkg, env, rows, mode, dtype, n_out, n_out2):
    """``susnet_featurize`` into buffers that start ONE ELEMENT past a 16-byte boundary (no vector store can be taken)."""
    L = pkg._lib
    spec = L.ObsSpec()
    spec.mode, spec.dtype = pkg.ObsConfig(mode).code, L.F32 if dtype == torch.float32 else L.U8
    # (a guard element on either side, filled with a value the kernel never writes)
    o1, o2 = torch.full((n_out + 8,), 7, dtype=dtype, device=DEV), torch.full((n_out2 + 8,), 7, dtype=dtype, device=DEV)
    assert o1.data_ptr() % 16 == 0 and o2.data_ptr() % 16 == 0
    spec.out, spec.out2 = o1.data_ptr() + o1.element_size(), o2.data_ptr() + o2.element_size()
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_featurize(env._h, rows.data_ptr(), env._ROW_DTYPES[rows.dtype], rows.shape[0], C.byref(spec), env._stream()))
    torch.cuda.synchronize()
    env.poll_errors()
    for o, n in ((o1, n_out), (o2, n_out2)):
        assert int(o[0]) == 7 and (o[1 + n:] == 7).all(), "a store outside the output"
    return o1[1:1 + n_out], o2[1:1 + n_out2]


@pytest.mark.parametrize("n_rows", [1, 63, 70, 129])
@pytest.mark.parametrize("name", list(GAMES))
def test_featurize_equals_the_restatement(pkg, envs, restated, name, n_rows):
    """Both modes, float32 and uint8 outputs, uint8 and int64 rows; 1 row (one lane), 63 and 70 (a ragged wave, a second wave of 6), 129
    (three waves); the same into buffers one element off the vector alignment; and plain ``"persp"`` of the same rows equals the masked
    output wherever the mask is 1 (one rotation, not a second one)."""
    env = envs[name]
    A, N = env.n_agents, env.n_rows
    rows_np, (want_sp, want_non) = restated[name]
    rows_np, want_sp, want_non = rows_np[:n_rows], want_sp[:n_rows], want_non[:n_rows]
    rows8 = torch.from_numpy(rows_np).to(DEV)
    plain, plain_non = env.featurize(rows8, pkg.ObsConfig("persp", dtype=torch.uint8))
    mask = want_sp[:, :, A + 2:]
    np.testing.assert_array_equal(np_(plain) * mask, want_sp[:, :, :A + 2])
    np.testing.assert_array_equal(np_(plain_non), want_non)
    for mode, with_mask in MODES:
        want = want_sp if with_mask else want_sp[:, :, :A + 2]
        for dtype in (torch.uint8, torch.float32):
            for rows in (rows8, rows8.to(torch.int64)):
                sp, non = env.featurize(rows, pkg.ObsConfig(mode, dtype=dtype))
                assert tuple(sp.shape) == (n_rows, A, A + 2 + int(with_mask), N, N)
                np.testing.assert_array_equal(np_(sp), want.astype(np_(sp).dtype), err_msg=f"{mode} {dtype} {rows.dtype}")
                np.testing.assert_array_equal(np_(non), want_non.astype(np_(non).dtype), err_msg=f"{mode} {dtype} {rows.dtype} non-spatial")
            sp, non = featurize_at_offset(pkg, env, rows8, mode, dtype, want.size, want_non.size)
            np.testing.assert_array_equal(np_(sp).reshape(want.shape), want.astype(np_(sp).dtype), err_msg=f"{mode} {dtype} offset output")
            np.testing.assert_array_equal(np_(non).reshape(want_non.shape), want_non.astype(np_(non).dtype), err_msg=f"{mode} {dtype} offset output 2")


def test_a_rejected_row_is_all_zeros_mask_channel_included(pkg, envs, restated):
    env = envs["tagging_1v4_j5"]
    rows_np, (want_sp, _) = restated["tagging_1v4_j5"]
    rows_np, want_sp = rows_np[:70].copy(), want_sp[:70].copy()
    rows_np[[5, 64], 0] = 9  # x of agent 0 outside the 9 x 9 grid
    want_sp[[5, 64]] = 0
    rows = torch.from_numpy(rows_np).to(DEV)
    with pytest.raises(IndexError, match="outside the grid"):
        env.featurize(rows, pkg.ObsConfig("persp_room_mask", dtype=torch.uint8))
    env.check_errors = False
    try:
        sp, _ = env.featurize(rows, pkg.ObsConfig("persp_room_mask", dtype=torch.uint8))
        torch.cuda.synchronize()
    finally:
        env.check_errors = True
    with pytest.raises(IndexError):
        env.poll_errors()
    np.testing.assert_array_equal(np_(sp), want_sp)


def test_step_reset_rollout_observe_refuse_the_modes(pkg, envs):
    env = envs["base14_1v2_j4"]
    cfg = pkg.ObsConfig("persp_room_mask", dtype=torch.uint8)
    with pytest.raises(Exception, match="SUSNET_OBS_PERSP_ROOM_MASK"):
        env.observe(cfg)
    with pytest.raises(Exception, match="SUSNET_OBS_PERSP_ROOM_MASK"):
        env.rollout(2, obs=cfg)


# ---- 2. windows: every state under its own mask ------------------------------------------------------------------------------------------
def test_each_state_of_a_window_carries_its_own_mask(pkg, envs, restated):
    env = envs["tagging_1v4_j5"]
    A = env.n_agents
    rows_np, _ = restated["tagging_1v4_j5"]
    win = rows_np[:128].reshape(64, 2, -1).copy()
    win[:, 0, 0:2], win[:, 1, 0:2] = (1, 1), (7, 7)  # the observer changes room between the two states
    win[:, :, 2 * A] = 1
    want_sp, want_non = pkg.features.room_mask_views(env, win, True)
    fz = pkg.PerspectiveFeaturizer(env, partially_observable=True)
    fz.fit(torch.from_numpy(win).to(DEV))
    assert tuple(fz.spatial.shape) == (64, 2, A, A + 3, 9, 9) and fz.spatial.dtype == torch.float32
    np.testing.assert_array_equal(np_(fz.spatial), want_sp.astype(np.float32))
    np.testing.assert_array_equal(np_(fz.non_spatial), want_non.astype(np.float32))
    m0, m1 = np_(fz.spatial[:, 0, 0, -1]), np_(fz.spatial[:, 1, 0, -1])
    assert (m0[:, :5, :5] == 1).all() and m0.sum() == 64 * 25 and (m1[:, 5:, 5:] == 1).all() and m1.sum() == 64 * 16
    views = fz.generate_featurized_states()
    assert len(views) == A and tuple(views[1][0].shape) == (64, 2, A + 3, 9, 9)


def test_fit_none_featurizes_the_current_state(pkg):
    env = make_env(pkg, "tagging_1v4_j5", batch=70, seed=11)
    env.reset()
    fz = pkg.PerspectiveFeaturizer(env, partially_observable=True, add_obs_mask_feature=False)
    fz.fit()
    raw = env.observe(raw8(pkg))
    want_sp, want_non = pkg.features.room_mask_views(env, raw.unsqueeze(1), False)
    np.testing.assert_array_equal(np_(fz.spatial), want_sp.astype(np.float32))
    np.testing.assert_array_equal(np_(fz.non_spatial), want_non.astype(np.float32))
    plain = pkg.PerspectiveFeaturizer(env)
    plain.fit()
    assert plain.config.mode == "persp" and tuple(plain.spatial.shape) == tuple(fz.spatial.shape)


# ---- 3. acting -------------------------------------------------------------------------------------------------------------------------------
def q_tolerance(want):
    return 2e-5 * float(want.abs().max())  # the project's Q-network tolerance (test_gpu_spatial.py, spatial_collect_util.KERNEL_TOLERANCE)


def test_windowed_rollout_acts_on_the_masked_views(pkg):
    B, T, ticks = 64, 2, 8
    env = make_env(pkg, "tagging_1v4_j5", batch=B, seed=5, max_time_steps=6)
    A = env.n_agents
    imp, crew = U.acting_models(pkg, A, 9, 2 * A + env.n_jobs, env.n_imposter_actions, env.n_crew_actions, DEV)
    fz = pkg.PerspectiveFeaturizer(env, partially_observable=True)
    policy = pkg.WindowedPolicyRollout(env, fz, imp, crew, sequence_length=T, mask_dead=True, kernels=True)
    assert policy.spatial_imposter is not None and policy.spatial_crew is not None and policy.spatial_imposter.C == A + 3
    host = U.HostRoomFeaturizer(pkg, env)
    policy.reset()
    excluded = compared = 0
    for tick in range(ticks):
        window = policy.window.clone()
        imp_mask, alive = env.imposter_mask.clone(), window[:, -1, 2 * A:3 * A].to(torch.bool)
        q = [x.clone() for x in policy.q_rows()]
        host.fit(window)
        with torch.no_grad():
            want = [torch.stack([m(s, x) for s, x in host.generate_featurized_states()], dim=1).reshape(B * A, -1) for m in (imp, crew)]
        tie = []
        for team, (got, w) in enumerate(zip(q, want)):
            tol = q_tolerance(w)
            err = float((got - w).abs().max())
            print(f"tick {tick} team {team}: max |error| {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol, (tick, team)
            top = w.topk(2, dim=1).values
            tie.append(((top[:, 0] - top[:, 1]) <= tol).view(B, A))
        actions = policy.step()[0].clone()
        greedy = torch.where(imp_mask, want[0].argmax(dim=1).view(B, A), want[1].argmax(dim=1).view(B, A)) * alive
        near = torch.where(imp_mask, tie[0], tie[1]) & alive
        assert torch.equal(actions[~near], greedy[~near]), tick
        excluded, compared = excluded + int(near.sum()), compared + near.numel()
    print(f"rows excluded for a near-tie: {excluded} of {compared}")
    assert excluded <= 0.05 * compared


def test_a_network_of_the_wrong_channel_count_is_refused_by_name(pkg):
    env = make_env(pkg, "tagging_1v4_j5", batch=8)
    A = env.n_agents
    imp, crew = U.acting_models(pkg, A, 9, 2 * A + env.n_jobs, env.n_imposter_actions, env.n_crew_actions, DEV, mask=False)  # A + 2 channels
    desc = pkg.policy.spatial_desc(imp)
    assert pkg.policy.spatial_feed_mismatch(env, pkg.PerspectiveFeaturizer(env, True, False), desc, env.n_imposter_actions) is None
    assert pkg.policy.spatial_feed_mismatch(env, pkg.PerspectiveFeaturizer(env), desc, env.n_imposter_actions) is None
    why = pkg.policy.spatial_feed_mismatch(env, pkg.PerspectiveFeaturizer(env, True), desc, env.n_imposter_actions)
    assert why is not None and "(channels, image size, non-spatial width, actions)" in why and str(A + 3) in why


# ---- 4. training -----------------------------------------------------------------------------------------------------------------------------
def _flat_exp_avg(tr, t):
    sd = tr.optimizer_state_dict(t)["state"]
    return torch.cat([sd[i]["exp_avg"].reshape(-1) for i in range(len(sd))]).clone()


def _train_two_steps(pkg, env, ring, models, idxs, featurizer, spatial):
    """-> (losses per step, first-step exp_avg per team, parameters per team after the last step) of a fresh trainer on copies of ``models``."""
    imp, crew = (copy.deepcopy(m) for m in models)
    tr = pkg.DeviceDQNTeamTrainer(env, imp, crew, [], 1e-3, 0.9, featurizer=featurizer, **({"spatial": True} if spatial else {}))
    assert tr.uses_spatial(ring) == spatial
    losses, first = [], None
    for idx in idxs:
        losses.append(tr.train_step_on_indices(ring, idx).clone())
        if first is None:
            first = [_flat_exp_avg(tr, t) for t in range(2)]
    torch.cuda.synchronize()
    return losses, first, [torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone() for m in (imp, crew)]


def _torch_two_steps_float64(pkg, env, ring, models, idxs):
    """``torch_train_step`` itself, twice, on the restated features in float64 (models, frozen targets and rewards in float64; Adam as the
    trainers build it: ``torch.optim.Adam(parameters, lr)``) -> the parameters per team."""
    class Host64(U.HostRoomFeaturizer):
        def fit(self, state_sequence):
            super().fit(state_sequence)
            self.spatial, self.non_spatial = self.spatial.double(), self.non_spatial.double()

    m64 = [copy.deepcopy(m).double() for m in models]
    targets = [copy.deepcopy(m) for m in m64]
    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in m64]
    sf, nf = Host64(pkg, env), Host64(pkg, env)
    for idx in idxs:
        sf.fit(ring.states[idx])
        nf.fit(ring.next_states[idx])
        pkg.torch_train_step(m64, targets, opts, 0.9, sf.generate_featurized_states(), nf.generate_featurized_states(), ring.actions[idx],
                             ring.rewards[idx].double(), ring.dones[idx], ring.imposters[idx])
    return [torch.cat([p.detach().reshape(-1) for p in m.parameters()]) for m in m64]


def test_trainer_learns_on_the_masked_views(pkg):
    """``DeviceDQNTeamTrainer(spatial=True)`` with the partially observable featurizer on a ring of 256 rows, n = 32, two steps, against
    ``torch_train_step`` on the restated features: the step is taken by ``susnet_spatial_train_step``; against a twin trainer on the
    float32 torch path the losses agree at every step (rtol 1e-4 / atol 1e-6) and the first step's gradients (Adam's exp_avg) lie within
    1e-4 of each team's max-abs; two runs leave identical bits; and the parameters after the two steps equal ``torch_train_step``'s,
    element by element, at tests/test_gpu_spatial_train.py's parameter tolerance for its torch comparison, rtol 1e-5 / atol 1e-6.

    The judge of that last comparison is ``torch_train_step`` run in FLOAT64 on the same restated features, because the float32 torch
    path's own error is larger than the tolerance on this batch.  Measured on the MI355X, parameters after the two steps (5251 imposter
    / 5238 crew elements), largest |difference| and elements outside rtol 1e-5 / atol 1e-6:
        kernels     against float64 torch   5.7e-8 / 1.4e-7     0 / 0
        float32 torch against float64 torch 8.7e-6 / 1.2e-7     2 / 0
        kernels     against float32 torch   8.7e-6 / 1.6e-7     2 / 0   (printed, not asserted: the first form of this test asserted it)
    The two elements have first-step gradients of 0 (kernels) against -2.98e-11 (float32 torch), and -2.3770e-4 on both sides, where the
    largest gradient is 1.17: Adam moves a parameter by about lr whatever its gradient's size (eps = 1e-8), so a cancelling sum that
    float32 torch leaves at 3e-11 moves the parameter by 3e-6 per step -- what test_gpu_spatial_train.py says above its own
    trainer-against-twin test, which does not compare parameters element by element for that reason.  With plain Perspective features
    the same trainer pair differs in 26 / 1 elements (up to 8.9e-5): a property of two float32 evaluations, not of the masked views."""
    env = make_env(pkg, "tagging_1v4_j5", batch=64, seed=8, max_time_steps=12)
    A, T = env.n_agents, 2
    ring = pkg.DeviceReplayBuffer(256, env.flattened_state_size, T, A, env.n_imposters, device=env.device)
    ring.populate_fused(env, 4)
    assert ring.size == 256
    models = U.acting_models(pkg, A, 9, 2 * A + env.n_jobs, env.n_imposter_actions, env.n_crew_actions, DEV, seeds=(21, 22))
    for m in models:
        m.train()
    g = torch.Generator(device=DEV)
    g.manual_seed(4)
    idxs = [torch.randint(0, ring.size, (32,), device=DEV, generator=g) for _ in range(2)]
    po = lambda: pkg.PerspectiveFeaturizer(env, partially_observable=True)
    losses, grads, params = _train_two_steps(pkg, env, ring, models, idxs, po(), True)
    want_losses, want_grads, twin = _train_two_steps(pkg, env, ring, models, idxs, U.HostRoomFeaturizer(pkg, env), False)
    for k in range(2):
        print(f"step {k}: losses {np_(losses[k])} torch {np_(want_losses[k])}")
        torch.testing.assert_close(losses[k], want_losses[k], rtol=1e-4, atol=1e-6)
    for t in range(2):
        scale = float(want_grads[t].abs().max())
        err = float((grads[t] - want_grads[t]).abs().max())
        print(f"team {t}: first-step exp_avg max |difference| {err:.3e} of max-abs {scale:.3e}")
        assert err <= 1e-4 * scale, t
    losses2, grads2, params2 = _train_two_steps(pkg, env, ring, models, idxs, po(), True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(losses + grads + params, losses2 + grads2 + params2))
    want = _torch_two_steps_float64(pkg, env, ring, models, idxs)

    def outside(a, b):
        diff = (a.double() - b.double()).abs()
        return f"max |difference| {float(diff.max()):.3e}, {int((diff > 1e-6 + 1e-5 * b.double().abs()).sum())} of {diff.numel()} outside"

    for t in range(2):
        print(f"team {t} parameters: kernels against float64 torch {outside(params[t], want[t])}; float32 torch against float64 torch "
              f"{outside(twin[t], want[t])}; kernels against float32 torch {outside(params[t], twin[t])}")
    for t in range(2):  # test_gpu_spatial_train.py's torch comparison of parameters: rtol 1e-5 / atol 1e-6
        torch.testing.assert_close(params[t].double(), want[t], rtol=1e-5, atol=1e-6)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_run_experiment_and_evaluate(pkg, tmp_path):
    env = make_env(pkg, "tagging_1v4_j5", batch=64, seed=7, max_time_steps=8)
    A = env.n_agents
    imp, crew = U.acting_models(pkg, A, 9, 2 * A + env.n_jobs, env.n_imposter_actions, env.n_crew_actions, DEV)
    fz = pkg.PerspectiveFeaturizer(env, partially_observable=True)
    pkg.run_experiment(env, num_steps=20, imposter_model=imp, crew_model=crew, components=[], sequence_length=2, replay_buffer_size=2048,
                       replay_prepopulate_steps=4, batch_size=32, gamma=0.9, scheduler_time_steps=10, experiment_base_dir=tmp_path,
                       learning_rate=1e-3, train_step_interval=5, target_update_interval=10, featurizer=fz)
    (run_dir,) = list(tmp_path.iterdir())
    config = json.loads((run_dir / "config.json").read_text())
    assert config["featurizer_type"] == "perspective_room_mask" and config["train_step"] == "susnet_spatial_train_step"
    assert config["imposter_model_args"]["n_channels"][0] == A + 3
    ckpt = pkg.SpatialDQN.load_from_checkpoint(run_dir / "imposter_spatial_dqn_100%.pt").to(DEV)
    got = pkg.evaluate(env, ckpt, crew, [], 16, epsilon=0.1, block_ticks=4, gamma=0.9, sequence_length=2, featurizer=fz)
    assert got["episodes"] >= env.batch
    for key in ("imposter_win_rate", "crew_win_rate", "truncation_rate"):
        assert math.isfinite(got[key]) and 0.0 <= got[key] <= 1.0, key
    table = pkg.train_loop.evaluate_checkpoints(run_dir, env, [], 8, featurizer=fz, sequence_length=2, block_ticks=4)
    assert "100%" in table and all(math.isfinite(s["imposter_win_rate"]) for s in table.values())


def test_a_plain_perspective_run_writes_what_it_always_wrote(pkg, tmp_path):
    env = make_env(pkg, "tagging_1v4_j5", batch=16, seed=7, max_time_steps=6)
    A = env.n_agents
    imp, crew = U.acting_models(pkg, A, 9, 2 * A + env.n_jobs, env.n_imposter_actions, env.n_crew_actions, DEV, mask=False)
    pkg.run_experiment(env, num_steps=5, imposter_model=imp, crew_model=crew, components=[], sequence_length=2, replay_buffer_size=256,
                       replay_prepopulate_steps=2, batch_size=8, gamma=0.9, scheduler_time_steps=5, experiment_base_dir=tmp_path,
                       learning_rate=1e-3, train_step_interval=5, target_update_interval=4, featurizer=pkg.PerspectiveFeaturizer(env))
    (run_dir,) = list(tmp_path.iterdir())
    assert json.loads((run_dir / "config.json").read_text())["featurizer_type"] == "perspective"
