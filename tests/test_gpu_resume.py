"""Resumable runs on the MI355X: a run that is stopped (``stop_after``), snapshotted (``run_state.pt``) and resumed into a fresh env and fresh
models (``resume_from``) must be the uninterrupted run, bit for bit.  The yardstick throughout is the uninterrupted run on the same machine
with the new arguments at their defaults -- the path the rest of the suite pins.

The scheme, per path: run A uninterrupted; run B1 the same call with ``stop_after=16``; run B2 with a fresh env and fresh models of OTHER
initial weights (anything left unrestored shows) and ``resume_from`` = B1's directory.  A and B1+B2 must agree on ``metrics.json``, the set of
checkpoint files and every tensor in them, the final ring with its cursors, the env's state blob and tick, both teams' parameters, target
parameters, Adam moments and step counts, ``EpisodeLog.records()``, the loss history, and the dropout counters.

Shapes: 96 envs (one full wave and a ragged one), 41 ticks with a train step every 5 (block boundaries 1, 6, .., 36, 41), target syncs every 10
and checkpoints at ticks 0, 10, 20, 30 (both on both sides of the cut at 16), a ring of 1024 rows that wraps before and after the cut
(96 x 41 transitions), 3 prepopulation ticks, batches of 32, an explicit seeded sample generator."""
import contextlib
import importlib
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 96
RUN = dict(num_steps=41, train_step_interval=5, target_update_interval=10, num_checkpoint_saves=5, replay_buffer_size=1024,
           replay_prepopulate_steps=3, batch_size=32, gamma=0.9, scheduler_time_steps=100, learning_rate=1e-3)
N_TRAIN = 9  # train ticks 0, 5, .., 40
CHECKPOINTS = ("0", "24", "48", "73", "100%")  # int(t * 100 / 41) at ticks 0, 10, 20, 30, and the end
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


# ---- the three paths: (env, imposter model, crew model, run_experiment keywords), models initialised under `model_seed` -----------------------
def _seeded(model_seed, build):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(model_seed)
        return build().to(DEV)


def _fused_env(pkg, seed=5, batch=B):
    kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
    return pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device=DEV, rng="philox", seed=seed,
                                             auto_reset=True, max_time_steps=9, obs=pkg.ObsConfig("flat", ["onehot_pos"]))


def fused_path(pkg, model_seed, batch=B):
    """ImposterTrainingGround 1v1 9 x 9 without walls, onehot_pos, the reference MLP stack, a random crew (its draws follow the handle's
    tick): the fused kernels act, susnet_dqn_train_step learns."""
    env = _fused_env(pkg, batch=batch)
    imp = pkg.policy.reference_imposter_mlp(env, ["onehot_pos"], seed=model_seed)
    return env, imp, None, dict(components=["onehot_pos"])


def dense_path(pkg, model_seed, batch=B):
    """Base 1v3 9 x 9, onehot_pos + alive_crew + closest_crew, windows of two states, both teams trained: the dense kernels act and learn."""
    T = 2
    env = pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9, max_time_steps=6,
                                 obs=pkg.ObsConfig("flat", COMPS3))
    F = env.obs.shape[-1]
    imp = _seeded(model_seed, lambda: pkg.MLP([T * F, 48, 24, env.n_imposter_actions]))
    crew = _seeded(model_seed + 1, lambda: pkg.MLP([T * F, 48, 24, env.n_crew_actions]))
    return env, imp, crew, dict(components=COMPS3, sequence_length=T)


def spatial_path(pkg, model_seed, batch=B):
    """Tagging 1v4 9 x 9 with the Global featurizer; small SpatialDQNs within the kernels' bounds: two RNN layers of 16 with dropout 0.2
    between them, windows of two states, both dropout seeds, the models left in training mode: the spatial kernels act and learn under
    dropout."""
    env = pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=14, auto_reset=True, grid_size=9, max_time_steps=6,
                                            obs=pkg.ObsConfig("raw", dtype=torch.uint8))
    fz = pkg.GlobalFeaturizer(env)
    _, planes, non = env._make_obs(fz.config, 1, rows=1)
    cfg = dict(input_image_size=env.n_rows, non_spatial_input_size=non.shape[-1] + env.n_agents, n_channels=[planes.shape[-3], 5, 3], strides=[1, 1],
               paddings=[1, 1], kernel_size=[3, 3], dilations=[1, 1], rnn_layers=2, rnn_hidden_dim=16, rnn_dropout=0.2, mlp_hidden_layer_dims=[8, 8])
    imp = _seeded(model_seed, lambda: pkg.SpatialDQN(**cfg, n_actions=env.n_imposter_actions))
    crew = _seeded(model_seed + 1, lambda: pkg.SpatialDQN(**cfg, n_actions=env.n_crew_actions))
    assert imp.training and crew.training
    return env, imp, crew, dict(components=[], sequence_length=2, featurizer=fz, rnn_dropout_seed=1, act_dropout_seed=2)


PATHS = {"fused": fused_path, "dense": dense_path, "spatial": spatial_path}
LEARNER = {"fused": "uses_hip", "dense": "uses_dense", "spatial": "uses_spatial"}


# ---- running, and reading what a run leaves behind -------------------------------------------------------------------------------------------
@contextlib.contextmanager
def spy_runs(pkg):
    """The ``_Run`` objects the entry points build while the block is open (ring, trainer, policy, episode log, losses are theirs)."""
    tl = pkg.train_loop
    real, seen = tl._Run, []

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append(self)

    tl._Run = Spy
    try:
        yield seen
    finally:
        tl._Run = real


def final_state(run):
    """What the issue lists, of one finished (or stopped) ``_Run``, on the host."""
    torch.cuda.synchronize()
    ring, tr, env = run.ring, run.trainer, run.env
    out = {f"ring.{f}": getattr(ring, f)[:ring.size].cpu() for f in RING_FIELDS}
    out["ring.idx_size"] = (ring.idx, ring.size)
    # (not env.obs: the fused path's rollout launches never write it, so the uninterrupted run ends with the observation of its
    # env.reset() there, while a restored env shows the restored state -- test_env_state_dict_restores_blob_tick_and_views checks that)
    out["env.blob"], out["env.tick"] = env._state.cpu(), env.tick
    for t in range(2):
        if tr.trained[t]:
            exp_avg, exp_avg_sq, step = tr.state_tensors(t)
            out[f"team{t}"] = {"flat": tr.flat[t].cpu(), "target_flat": tr.target_flat[t].cpu(), "exp_avg": exp_avg.cpu(), "exp_avg_sq": exp_avg_sq.cpu(),
                               "step": step.cpu(), "module": [p.detach().cpu() for p in tr.models[t].parameters()],
                               "target_module": [p.detach().cpu() for p in tr.targets[t].parameters()],
                               "modes": (tr.models[t].training, tr.targets[t].training)}
    out["records"] = {k: torch.as_tensor(np.asarray(v)) for k, v in run.episode_log.records().items()}
    out["losses"] = run.losses.cpu()
    out["act_ticks"], out["dropout_steps"] = getattr(run.policy, "act_ticks", None), tr.dropout_steps
    return out


def same(a, b, where=""):
    """Equal structure, tensors equal bit for bit (compared as bytes: a NaN equals itself), everything else equal."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, where
        assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), where
    elif isinstance(a, torch.nn.Module):
        same(a.state_dict(), b.state_dict(), where)
    else:
        assert a == b, (where, a, b)


def same_directory(a, b, teams):
    """config.json but for the base directory, metrics.json, and the checkpoints: first the SET of files, then every tensor."""
    names = {p.name for p in a.iterdir()} - {"run_state.pt"}
    assert names == {p.name for p in b.iterdir()} - {"run_state.pt"}
    kind = "spatial_dqn" if any("spatial_dqn" in n for n in names) else "mlp"
    assert names == {"config.json", "metrics.json"} | {f"{team}_{kind}_{p}.pt" for team in teams for p in CHECKPOINTS}
    ca, cb = (json.loads((d / "config.json").read_text()) for d in (a, b))
    assert {k: v for k, v in ca.items() if k != "experiment_base_dir"} == {k: v for k, v in cb.items() if k != "experiment_base_dir"}
    assert (a / "metrics.json").read_text() == (b / "metrics.json").read_text()
    metrics = json.loads((a / "metrics.json").read_text())
    assert len(metrics["imposter_loss"]) == N_TRAIN and len(metrics["avg_imposter_returns"]) > 0
    for name in sorted(n for n in names if n.endswith(".pt")):
        x, y = (torch.load(d / name, map_location="cpu", weights_only=False) for d in (a, b))
        same(x, y, name)


def only(directory):
    (entry,) = list(directory.iterdir())
    return entry


def listing(directory):
    return sorted((p.name, p.read_bytes()) for p in directory.iterdir())


def run(pkg, path, base, model_seed=3, batch=B, resume_from=None, **extra):
    """One ``run_experiment`` call on ``path`` with a fresh env, fresh models and a fresh generator seeded alike.  Returns (the run's
    directory, its ``_Run``)."""
    env, imp, crew, kw = PATHS[path](pkg, model_seed, batch)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    with spy_runs(pkg) as seen:
        pkg.run_experiment(env, imposter_model=imp, crew_model=crew, experiment_base_dir=base, generator=gen, resume_from=resume_from,
                           **dict(RUN, **kw, **extra))
    (r,) = seen
    assert getattr(r.trainer, LEARNER[path])(r.ring), f"the {path} path is meant to learn through its HIP step"
    return (resume_from if resume_from is not None else only(base)), r


_A = {}


@pytest.fixture(scope="module")
def uninterrupted(pkg, tmp_path_factory):
    """Run A per path, made once: ``uninterrupted(path)`` -> (directory, final state, teams)."""
    def get(path):
        if path not in _A:
            d, r = run(pkg, path, tmp_path_factory.mktemp(f"A_{path}"))
            assert not (d / "run_state.pt").exists()  # the arguments at their defaults: no snapshot
            state = final_state(r)
            assert state["ring.idx_size"] == ((B * (41 + 3)) % 1024, 1024) and state["records"]["count"] > 0 and state["env.tick"] > 0
            _A[path] = (d, state, ["imposter"] if path == "fused" else ["imposter", "crew"])
        return _A[path]

    yield get
    _A.clear()


# ---- 1-3. the three-run scheme on every path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "dense", "spatial"])
def test_a_stopped_and_resumed_run_is_the_uninterrupted_run(pkg, tmp_path, uninterrupted, path):
    dir_a, want, teams = uninterrupted(path)
    dir_b, b1 = run(pkg, path, tmp_path / "b", stop_after=16)
    stopped = final_state(b1)
    # the stopped run: at tick 16, the checkpoints of ticks 0 and 10 written, no 100% checkpoint, no metrics.json, one snapshot
    kind = "spatial_dqn" if path == "spatial" else "mlp"
    assert {p.name for p in dir_b.iterdir()} == {"config.json", "run_state.pt"} | {f"{t}_{kind}_{p}.pt" for t in teams for p in ("0", "24")}
    assert not b1.finished and stopped["records"]["count"] < want["records"]["count"]
    snap = pkg.read_run_state(dir_b)
    assert snap["completed_ticks"] == 16 and snap["train_steps"] == 4 and tuple(snap["losses"].shape) == (4, 2)
    # resumed into a fresh env and fresh models of other initial weights
    d, b2 = run(pkg, path, None, model_seed=77, resume_from=dir_b)
    assert d == dir_b and b2.finished
    got = final_state(b2)
    same(got, want, path)
    same_directory(dir_a, dir_b, teams)
    if path == "spatial":  # acting and learning under dropout: the two counters went on from the snapshot's
        assert snap["policy"]["act_ticks"] == 16 and snap["trainer"]["dropout_steps"] == 4
        assert got["act_ticks"] == want["act_ticks"] == 41 and got["dropout_steps"] == want["dropout_steps"] == N_TRAIN
        config = json.loads((dir_b / "config.json").read_text())
        assert config["train_step"] == "susnet_spatial_train_step" and config["act_dropout_seed"] == 2 and config["rnn_dropout_seed"] == 1
        assert all(m.training for m in b2.trainer.models)
    # the resumed models are views of the trainer's flat buffers still, and hold what the uninterrupted run's hold
    for t, tr in enumerate(b2.trainer.trained):
        if tr:
            flat, off = b2.trainer.flat[t], 0
            for p in b2.trainer.models[t].parameters():
                assert p.data_ptr() == flat.data_ptr() + 4 * off
                off += p.numel()


# ---- 4. a sweep, stopped and resumed as one ---------------------------------------------------------------------------------------------------
VARIANTS = [{"gamma": 0.99, "name": "g0.99", "seed": 1}, {"gamma": 0.9, "name": "g0.9", "seed": 2}, {"gamma": 0.8, "seed": 3}]
MEMBER_DIRS = ("g0.99", "g0.9", "2")


def sweep(pkg, base, model_seed=1, **extra):
    comps = ["onehot_pos"]
    common = dict(RUN, components=comps, train_crew=False)
    common.pop("gamma")
    with spy_runs(pkg) as seen:
        pkg.run_sweep(lambda seed: _fused_env(pkg, seed=seed), VARIANTS,
                      imposter_model_factory=lambda env: pkg.policy.reference_imposter_mlp(env, comps, seed=model_seed), crew_model_factory=None,
                      experiment_base_dir=base, **common, **extra)
    assert len(seen) == 3
    return seen


def test_a_sweep_is_stopped_and_resumed_as_one(pkg, tmp_path):
    runs_a = sweep(pkg, tmp_path / "a")
    want = [final_state(r) for r in runs_a]
    assert not any(same_or_not(want[0], w) for w in want[1:]), "the variants are different runs"
    b1 = sweep(pkg, tmp_path / "b", stop_after=16)
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(MEMBER_DIRS)
    stamp = only(tmp_path / "b" / "g0.9").name
    for name in MEMBER_DIRS:  # one file per member directory, all at the same boundary
        assert pkg.read_run_state(tmp_path / "b" / name / stamp)["completed_ticks"] == 16
        assert not (tmp_path / "b" / name / stamp / "metrics.json").exists()
    assert not any(r.finished for r in b1)
    b2 = sweep(pkg, tmp_path / "elsewhere", model_seed=55, resume_from=tmp_path / "b" / stamp)  # the members' common base with the timestamp
    assert not (tmp_path / "elsewhere").exists(), "a resumed sweep continues in its members' directories"
    for k, name in enumerate(MEMBER_DIRS):
        same(final_state(b2[k]), want[k], name)
        same_directory(only(tmp_path / "a" / name), tmp_path / "b" / name / stamp, ["imposter"])


def same_or_not(a, b):
    try:
        same(a, b)
    except AssertionError:
        return False
    return True


# ---- 5. two cuts ------------------------------------------------------------------------------------------------------------------------------
def test_a_snapshot_taken_by_a_resumed_run_is_complete(pkg, tmp_path, uninterrupted):
    dir_a, want, teams = uninterrupted("fused")
    d, _ = run(pkg, "fused", tmp_path / "b", stop_after=6)
    assert pkg.read_run_state(d)["completed_ticks"] == 6
    _, r = run(pkg, "fused", None, model_seed=41, resume_from=d, stop_after=21)
    assert pkg.read_run_state(d)["completed_ticks"] == 21 and not r.finished and not (d / "metrics.json").exists()
    with pytest.raises(ValueError, match="stop_after = 21 stops at 21 completed ticks, and the resumed run has 21 behind it"):
        run(pkg, "fused", None, model_seed=42, resume_from=d, stop_after=21)
    _, r = run(pkg, "fused", None, model_seed=43, resume_from=d)
    same(final_state(r), want, "two cuts")
    same_directory(dir_a, d, teams)


# ---- 6. snapshot_interval without a stop ------------------------------------------------------------------------------------------------------
def test_snapshot_interval_leaves_the_run_as_it_is_and_its_last_snapshot_resumes(pkg, tmp_path, uninterrupted):
    dir_a, want, teams = uninterrupted("dense")
    d, r = run(pkg, "dense", tmp_path / "b", snapshot_interval=10)
    assert r.finished
    same(final_state(r), want, "snapshot_interval=10")
    same_directory(dir_a, d, teams)
    assert sorted(p.name for p in d.iterdir() if "run_state" in p.name) == ["run_state.pt"]  # one file, the latest; no temporary left
    assert pkg.read_run_state(d)["completed_ticks"] == 31  # boundaries 11, 21, 31: the last one written lies before the end
    _, r2 = run(pkg, "dense", None, model_seed=9, resume_from=d)
    same(final_state(r2), want, "resumed from the last snapshot")
    same_directory(dir_a, d, teams)


# ---- the refusals: nothing is written ---------------------------------------------------------------------------------------------------------
def test_a_resume_with_other_arguments_is_refused_and_leaves_the_directory_untouched(pkg, tmp_path):
    d, _ = run(pkg, "fused", tmp_path / "b", stop_after=16)
    before = listing(d)
    with pytest.raises(ValueError, match=r"gamma is 0\.8 in this call and 0\.9 in the run's config\.json"):
        run(pkg, "fused", None, resume_from=d, gamma=0.8)
    assert listing(d) == before
    with pytest.raises(ValueError, match=r"batch is 64 in this call and 96 in the run's config\.json"):
        run(pkg, "fused", None, batch=64, resume_from=d)
    assert listing(d) == before
    with pytest.raises(ValueError, match=r"drew its samples from a generator of its own"):  # (config.json does not say: the snapshot does)
        env, imp, crew, kw = fused_path(pkg, 3)
        pkg.run_experiment(env, imposter_model=imp, crew_model=crew, resume_from=d, **dict(RUN, **kw))
    assert listing(d) == before
    with pytest.raises(FileNotFoundError, match=r"there is no run_state\.pt"):
        (tmp_path / "empty").mkdir()
        (tmp_path / "empty" / "config.json").write_bytes((d / "config.json").read_bytes())
        run(pkg, "fused", None, resume_from=tmp_path / "empty")
    assert [p.name for p in (tmp_path / "empty").iterdir()] == ["config.json"]


# ---- the env's own state_dict: both forms of the tick, the refusals ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_tick", [False, True])
def test_env_state_dict_restores_blob_tick_and_views(pkg, device_tick):
    def make(seed=9, batch=B, max_time_steps=6):
        return pkg.BatchedFourRoomEnv(1, 3, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9,
                                      max_time_steps=max_time_steps, obs=pkg.ObsConfig("flat", COMPS3))

    a = make()
    a.reset()
    a.device_tick(device_tick)
    for _ in range(7):
        a.step(a.sample_actions())
    sd = a.state_dict()
    assert sd["tick"] == 7 and sd["device_tick"] is device_tick and sd["blob"].device.type == "cpu"
    b = make()
    b.load_state_dict(sd)
    torch.cuda.synchronize()
    assert b.tick == 7 and b.reset_generation == a.reset_generation
    for name in ("_state", "obs", "agent_positions", "alive_agents", "imposter_mask", "job_positions", "completed_jobs", "_metrics", "_t"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for _ in range(5):  # the action stream follows the restored tick, the dynamics the restored cursors
        acts = [e.sample_actions().clone() for e in (a, b)]
        assert torch.equal(*acts)
        for e, x in zip((a, b), acts):
            e.step(x)
    torch.cuda.synchronize()
    assert a.tick == b.tick == 12 and torch.equal(a._state, b._state) and torch.equal(a.lifetime_totals(), b.lifetime_totals())
    for other, field in ((make(batch=64), "batch"), (make(seed=10), "seed"), (make(max_time_steps=7), "max_time_steps")):
        blob = other._state.clone()
        with pytest.raises(ValueError, match=rf"saved from another configuration: {field} is "):
            other.load_state_dict(sd)
        assert torch.equal(other._state, blob)
    other_abi = dict(sd, identity=dict(sd["identity"], abi_version=sd["identity"]["abi_version"] + 1))
    with pytest.raises(ValueError, match="SUSNET_ABI_VERSION is "):
        make().load_state_dict(other_abi)


def test_a_numpy_tape_env_is_refused(pkg):
    env = pkg.BatchedFourRoomEnv(1, 3, 5, batch=2, device=DEV, rng="numpy", seed=0, auto_reset=True, grid_size=9)
    with pytest.raises(ValueError, match="rng='numpy'.*a tape is the caller's"):
        env.state_dict()
    with pytest.raises(ValueError, match="rng='numpy'.*a tape is the caller's"):
        env.load_state_dict({})
