"""Shared reading and checking of tests/golden/spatial_train/train_*.npz (written by tests/golden/generate_train_spatial.py from the reference's
own DQNTeamTrainer.train_step, SpatialDQN, featurizers and torch.optim.Adam): used by the CPU test of the torch path and the GPU test of
susnet_spatial_train_step.  The criteria are train_fixtures.py's: first-step gradients (exp_avg / (1 - beta1)) within 1e-4 of each
tensor's max-abs; parameters, here after EVERY step, ||p - p_ref|| <= 1e-3 ||p_ref - p_init|| per tensor; Adam step counts exact."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_train")
TEAMS = ("imposter", "crew")
NAMES = {"global": "train_global_t2", "perspective": "train_perspective_t3"}


def load(name):
    d = np.load(os.path.join(GOLDEN, NAMES[name] + ".npz"))
    return json.loads(str(d["meta"])), d


def step_indices(meta, d):
    idx, out, off = d["indices"].astype(np.int64), [], 0
    for bs in meta["batch_sizes"]:
        out.append(idx[off:off + bs])
        off += bs
    return out


def models_from(pkg, meta, d):
    """[imposter, crew] SpatialDQN at the fixture's initial parameters."""
    out = []
    for team in TEAMS:
        m = pkg.SpatialDQN(**dict(meta["config"], n_actions=meta["n_actions"][team]))
        m.load_state_dict({k[len(f"init::{team}::"):]: torch.tensor(d[k]) for k in d.files if k.startswith(f"init::{team}::")})
        out.append(m)
    return out


def agent_views(d, prefix, idx):
    """One (spatial [n, T, C, N, N], non_spatial [n, T, Fn]) per agent of the recorded reference featurizer output at ring rows idx."""
    sp, ns = torch.tensor(d[prefix + "spatial"][idx]).float(), torch.tensor(d[prefix + "non_spatial"][idx])
    return [(sp if sp.dim() == 5 else sp[:, :, i], ns[:, :, i]) for i in range(ns.shape[2])]


def check_step(d, step, models, exp_avg=None):
    """The parameters after step `step` (0-based) per tensor, and after the first step Adam's exp_avg ([team] -> {name: array}, or None)."""
    for team, m in zip(TEAMS, models):
        for n, p in m.named_parameters():
            ref, init = d[f"step{step}::{team}::{n}"].astype(np.float64), d[f"init::{team}::{n}"].astype(np.float64)
            moved, err = float(np.linalg.norm(ref - init)), float(np.linalg.norm(p.detach().cpu().numpy().astype(np.float64) - ref))
            assert err <= 1e-3 * moved or (moved == 0.0 and err == 0.0), f"step {step} {team} {n}: {err:.3e} vs moved {moved:.3e}"
    if step == 0 and exp_avg is not None:
        for t, team in enumerate(TEAMS):
            for n, got in exp_avg[t].items():
                ref = d[f"first_exp_avg::{team}::{n}"].astype(np.float64)
                scale = max(float(np.abs(ref).max()), 1e-30)
                err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()) / scale
                assert err <= 1e-4, f"{team} {n}: first-step gradient off by {err:.2e} of max-abs"
