"""What run_experiment() and run_sweep() leave on disk for each of the four kinds of run -- flat, flat on windows (the dense path), SpatialDQN,
and the flat / SpatialDQN sweeps -- pinned as literals: the whole config.json in key order, the set of files of the run directory and the
lengths of the histories in metrics.json.  The runs are the smallest the loop tests use; what the steps compute is pinned elsewhere
(test_gpu_train_loop.py, test_gpu_sweep.py, test_gpu_spatial_sweep.py, test_gpu_spatial_collect.py, test_gpu_window.py)."""
import importlib
import json

import pytest
import torch

from test_gpu_spatial_sweep import _raw_env, _spatial_models
from test_gpu_sweep import _env_1v1
from test_gpu_train_loop import _game
from test_gpu_window import seeded_mlp, tagging_1v4
from train_exact import DEV

pytestmark = pytest.mark.gpu

# num_steps = 11, a train step every 5 ticks: train ticks 0, 5, 10; checkpoints at linspace(0, 11, 4) = ticks 0, 2, 5, 8 and at the end
RUN = dict(num_steps=11, batch_size=8, train_step_interval=5, target_update_interval=10, scheduler_time_steps=100, learning_rate=1e-3)
N_TRAIN = 3
PROGRESS = ("0", "18", "45", "72", "100%")
INFO = ("imp_killed_crew", "imp_voted_out", "crew_voted_out", "sabotaged_jobs", "completed_jobs", "total_stalemates", "total_time_steps",
        "imposter_won", "crew_won")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _config(base, num_batch, imposter_args, crew_args, kinds, featurizer_type, T, ring_rows, prepopulate, gamma, train_crew, extras):
    """config.json as the ordered (key, value) pairs run_experiment writes (train.py:185-211), then the kind's extras."""
    return [("num_steps", 11), ("batch", num_batch), ("imposter_model_args", imposter_args), ("crew_model_args", crew_args),
            ("imposter_model_type", kinds[0]), ("crew_model_type", kinds[1]), ("featurizer_type", featurizer_type), ("sequence_length", T),
            ("replay_buffer_size", ring_rows), ("replay_prepopulate_steps", prepopulate), ("batch_size", 8), ("gamma", gamma),
            ("scheduler_start_eps", 1.0), ("scheduler_end_eps", 0.05), ("scheduler_time_steps", 100), ("train_imposter", True),
            ("train_crew", train_crew), ("experiment_base_dir", str(base)), ("optimizer_type", "adam"), ("learning_rate", 0.001),
            ("train_step_interval", 5), ("target_update_interval", 10)] + list(extras)


def _files(kind, teams):
    return {"config.json", "metrics.json"} | {f"{team}_{kind}_{p}.pt" for team in teams for p in PROGRESS}


def _check_run(run_dir, want_config, want_files, handler):
    config = list(json.loads((run_dir / "config.json").read_text()).items())
    files = {p.name for p in run_dir.iterdir()}
    saved = json.loads((run_dir / "metrics.json").read_text())
    lengths = {key: len(v) for key, v in saved.items()}
    print(config, sorted(files), lengths, sep="\n")
    assert config == want_config
    assert files == want_files
    assert lengths["imposter_loss"] == lengths["crew_loss"] == N_TRAIN
    n_episodes = lengths["avg_imposter_returns"]
    assert n_episodes > 0 and lengths["avg_crew_returns"] == n_episodes
    assert all(lengths[key] == n_episodes for key in INFO)  # (per_episode_info: one entry per episode, the reference's shape)
    assert set(lengths) == {"avg_imposter_returns", "avg_crew_returns", "imposter_loss", "crew_loss", *INFO}
    assert {m.value: v for m, v in handler.metrics.items()} == saved


def _only(directory):
    (entry,) = list(directory.iterdir())
    return entry


def test_flat_run_experiment_on_a_compiled_in_layout(pkg, tmp_path):
    env, comps = _game(pkg, "1v1", batch=64)
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    handler = pkg.run_experiment(env, imposter_model=imp, crew_model=None, components=comps, replay_buffer_size=64 * 64, replay_prepopulate_steps=4,
                                 gamma=0.9, experiment_base_dir=tmp_path, **RUN)
    want = _config(tmp_path, 64, {"layer_dims": [36, 256, 128, 64, 16, 6]}, None, ("mlp", "random"), "flat:onehot_pos", 1, 4096, 4, 0.9, True, [])
    _check_run(_only(tmp_path), want, _files("mlp", ["imposter"]), handler)


def test_flat_run_experiment_on_windows_takes_the_dense_path(pkg, tmp_path):
    T, comps = 2, ["onehot_pos"]
    env = tagging_1v4(pkg, 64, seed=13, max_time_steps=6)  # (every env ends an episode within the 11 ticks)
    F = env.obs.shape[-1]
    assert F == 90
    imp = seeded_mlp(pkg, [T * F, 128, 64, 16, env.n_imposter_actions], seed=3)
    crew = seeded_mlp(pkg, [T * F, 64, 16, env.n_crew_actions], seed=4)
    handler = pkg.run_experiment(env, imposter_model=imp, crew_model=crew, components=comps, sequence_length=T, replay_buffer_size=64 * 64,
                                 replay_prepopulate_steps=8, gamma=0.9, experiment_base_dir=tmp_path, **RUN)
    want = _config(tmp_path, 64, {"layer_dims": [180, 128, 64, 16, 11]}, {"layer_dims": [180, 64, 16, 10]}, ("mlp", "mlp"), "flat:onehot_pos", 2, 4096,
                   8, 0.9, True, [])
    _check_run(_only(tmp_path), want, _files("mlp", ["imposter", "crew"]), handler)


def _spatial_args(image, non_spatial, channels, n_actions):
    """SpatialDQN.config of test_gpu_spatial_sweep._spatial_models."""
    return {"input_image_size": image, "non_spatial_input_size": non_spatial, "n_channels": [channels, 6], "strides": [1], "paddings": [1],
            "dilations": [1], "kernel_size": [3, 3], "rnn_layers": 1, "rnn_hidden_dim": 16, "rnn_dropout": 0.0, "mlp_hidden_layer_dims": [12],
            "n_actions": n_actions}


def test_spatial_run_experiment(pkg, tmp_path):
    """Global featurizer, T = 2, base 1v4 with 5 jobs on 9 x 9 (the notebook's game), the sweep tests' small network."""
    env = pkg.BatchedFourRoomEnv(1, 4, 5, batch=8, device=DEV, rng="philox", seed=70, auto_reset=True, grid_size=9,
                                 obs=pkg.ObsConfig("raw", dtype=torch.uint8), max_time_steps=6)
    imp, crew = _spatial_models(pkg, env, 3)
    handler = pkg.run_experiment(env, imposter_model=imp, crew_model=crew, components=[], sequence_length=2, replay_buffer_size=8 * 16,
                                 replay_prepopulate_steps=3, gamma=0.9, experiment_base_dir=tmp_path, featurizer=pkg.GlobalFeaturizer(env), **RUN)
    want = _config(tmp_path, 8, _spatial_args(9, 15, 7, 7), _spatial_args(9, 15, 7, 6), ("spatial_dqn", "spatial_dqn"), "global", 2, 128, 3, 0.9, True,
                   [("train_step", "susnet_spatial_train_step"), ("rnn_dropout_seed", None)])
    _check_run(_only(tmp_path), want, _files("spatial_dqn", ["imposter", "crew"]), handler)


VARIANTS = [{"gamma": 0.9, "name": "g0.9", "seed": 1}, {"gamma": 0.8, "seed": 2}]


def test_flat_run_sweep(pkg, tmp_path):
    comps = ["onehot_pos"]
    handlers = pkg.run_sweep(lambda seed: _env_1v1(pkg, seed, comps, batch=64), VARIANTS,
                             imposter_model_factory=lambda env: pkg.policy.reference_imposter_mlp(env, comps, seed=1), crew_model_factory=None,
                             components=comps, replay_buffer_size=64 * 16, replay_prepopulate_steps=4, train_crew=False, experiment_base_dir=tmp_path,
                             **RUN)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["1", "g0.9"]
    for name, gamma, seed, handler in (("g0.9", 0.9, 1, handlers[0]), ("1", 0.8, 2, handlers[1])):
        want = _config(tmp_path, 64, {"layer_dims": [36, 256, 128, 64, 16, 6]}, None, ("mlp", "random"), "flat:onehot_pos", 1, 1024, 4, gamma, False,
                       [("seed", seed)])
        _check_run(_only(tmp_path / name), want, _files("mlp", ["imposter"]), handler)


def test_spatial_run_sweep(pkg, tmp_path):
    handlers = pkg.run_sweep(lambda seed: _raw_env(pkg, seed), VARIANTS, imposter_model_factory=lambda env: _spatial_models(pkg, env, 1)[0],
                             crew_model_factory=lambda env: _spatial_models(pkg, env, 1)[1], components=[], sequence_length=2,
                             replay_buffer_size=8 * 16, replay_prepopulate_steps=3, experiment_base_dir=tmp_path,
                             featurizer_factory=lambda env: pkg.GlobalFeaturizer(env), **RUN)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["1", "g0.9"]
    for name, gamma, seed, handler in (("g0.9", 0.9, 1, handlers[0]), ("1", 0.8, 2, handlers[1])):
        want = _config(tmp_path, 8, _spatial_args(9, 13, 6, 7), _spatial_args(9, 13, 6, 6), ("spatial_dqn", "spatial_dqn"), "global", 2, 128, 3, gamma,
                       True, [("seed", seed), ("rnn_dropout_seed", None), ("train_step", "susnet_spatial_train_sweep")])
        _check_run(_only(tmp_path / name), want, _files("spatial_dqn", ["imposter", "crew"]), handler)
