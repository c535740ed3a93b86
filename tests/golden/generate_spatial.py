#!/usr/bin/env python3
"""Golden vectors for the SpatialDQN kernels (container only): the UNMODIFIED reference `SpatialDQN` (src/models/dqn.py:205-301) on the
UNMODIFIED reference featurizers' output (src/features/model_ready.py) over windows of a seeded random rollout of the reference env.
Stored as data: the parameters by state_dict key, the featurizer's `(spatial, non_spatial)` inputs of every agent's view and the module's
eval-mode outputs.

    python tests/golden/generate_spatial.py        # rewrites tests/golden/spatial/*.npz
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()
import torch  # noqa: E402

from generate_golden import GRID14, make_env  # noqa: E402
from src.features.model_ready import GlobalFeaturizer, PerspectiveFeaturizer  # noqa: E402
from src.models.dqn import SpatialDQN  # noqa: E402

OUT = os.path.join(HERE, "spatial")


def windows_of_a_rollout(env, T, n_windows, seed, every):
    """`n_windows` windows [T, S] of flattened states, `every` steps apart, from a random rollout: the trainer's window (train.py:318-322,
    388-389, 441-445: the first state T times, rolled one state on per step, refilled after a reset)."""
    np.random.seed(seed)
    state, _ = env.reset()
    window = np.stack([np.asarray(env.flatten_state(state), dtype=np.float64)] * T)
    out, step = [], 0
    while len(out) < n_windows:
        if step % every == 0:
            out.append(window.copy())
        state, _, done, trunc, _ = env.step(env.sample_actions())
        if done or trunc:
            state, _ = env.reset()
            window = np.stack([np.asarray(env.flatten_state(state), dtype=np.float64)] * T)
        else:
            window = np.roll(window, -1, axis=0)
            window[-1] = np.asarray(env.flatten_state(state), dtype=np.float64)
        step += 1
    return np.stack(out)


def every_parameter_matters(model, seed):
    """Default PReLU slopes are all 0.25 and default biases small (generate_models.py: coordinate_mlp does the same)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, mod in enumerate(m for m in model.modules() if isinstance(m, torch.nn.PReLU)):
            mod.weight.fill_((0.1, 0.3, 0.5, 0.7, 0.2, 0.4)[i])
        for name, p in model.named_parameters():
            if "bias" in name:
                p.copy_((torch.rand(p.shape, generator=gen) - 0.5) * 0.6)


def dump(name, spec, featurizer_cls, cfg_of, T, n_windows, seed, every):
    env = make_env(spec)
    feat = featurizer_cls(env)
    seq = torch.tensor(windows_of_a_rollout(env, T, n_windows, seed, every))
    feat.fit(seq)
    views = feat.generate_featurized_states()  # one (spatial [B, T, C, N, N], non_spatial [B, T, Fn]) per agent
    spatial = torch.stack([v[0].detach().float() for v in views], dim=2)          # [B, T, A, C, N, N]
    non_spatial = torch.stack([v[1].detach().float() for v in views], dim=2)      # [B, T, A, Fn]
    cfg = cfg_of(env, int(spatial.shape[3]), int(spatial.shape[-1]), int(non_spatial.shape[-1]))
    arrays, outputs = {}, {}
    for team, n_actions, mseed in (("imposter", env.n_imposter_actions, seed + 100), ("crew", env.n_crew_actions, seed + 200)):
        torch.manual_seed(mseed)
        model = SpatialDQN(**dict(cfg, n_actions=int(n_actions)))
        every_parameter_matters(model, mseed)
        model.eval()
        with torch.no_grad():
            outputs[team] = torch.stack([model(spatial[:, :, i], non_spatial[:, :, i]) for i in range(spatial.shape[2])], dim=1).numpy()  # [B, A, n]
        arrays.update({f"{team}::{k}": v.detach().numpy() for k, v in model.state_dict().items()})
    meta = dict(spec, featurizer=featurizer_cls.__name__, T=T, seed=seed, config=cfg, n_agents=int(env.n_agents), n_jobs=int(env.n_jobs),
                n_actions={"imposter": int(env.n_imposter_actions), "crew": int(env.n_crew_actions)})
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), spatial=spatial.numpy().astype(np.uint8), non_spatial=non_spatial.numpy(),
                        q_imposter=outputs["imposter"], q_crew=outputs["crew"], **arrays)
    assert np.array_equal(spatial.numpy().astype(np.uint8).astype(np.float32), spatial.numpy()), "the planes are small whole numbers"
    print(name, "inputs", tuple(spatial.shape), tuple(non_spatial.shape), "bytes", os.path.getsize(path))


def main():
    # (a) the network of notebooks/experiment.ipynb at its game's sizes: 1v4, 5 jobs, 9x9, GlobalFeaturizer, T = 6.  On the BASE game: the
    # reference's GlobalFeaturizer raises on FourRoomEnvWithTagging (tagging.py:15-25 orders `state_fields` differently from the tuple its
    # own observation_space unflattens, so component.py:120-124 reads the alive flags as job positions), so there is no reference output
    # to record on the tagging game; the planes are the same A + 2 = 7, the non-spatial row is [alive, job status, onehot(agent)] = 15 wide
    dump("base_1v4_global_t6", dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=4, n_jobs=5)), GlobalFeaturizer,
         lambda env, C, N, Fn: dict(input_image_size=N, non_spatial_input_size=Fn, n_channels=[C, 5, 3], strides=[1, 1], paddings=[1, 1],
                                    kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=64, rnn_dropout=0.0,
                                    mlp_hidden_layer_dims=[16, 16]),
         T=6, n_windows=40, seed=31, every=7)
    # (b) the shape of the windowed-rollout test: base 1v2, 4 jobs, 14x14, PerspectiveFeaturizer, T = 3
    dump("base14_1v2_persp_t3", dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=2, n_jobs=4), grid=GRID14.astype(int).tolist()),
         PerspectiveFeaturizer,
         lambda env, C, N, Fn: dict(input_image_size=N, non_spatial_input_size=Fn, n_channels=[C, 6, 8], strides=[1, 1], paddings=[1, 1],
                                    kernel_size=[3, 3], dilations=[1, 1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0,
                                    mlp_hidden_layer_dims=[12]),
         T=3, n_windows=40, seed=32, every=5)


if __name__ == "__main__":
    main()
