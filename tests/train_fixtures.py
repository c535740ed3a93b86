"""Shared reading and checking of tests/golden/model_train_*.npz (written by tests/golden/generate_train.py from the reference's own
DQNTeamTrainer.train_step and torch.optim.Adam): used by the CPU test of the torch path and the GPU test of the HIP path."""
import glob
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEAMS = ("imposter", "crew")
BETA1 = 0.9


def fixture_names():
    return sorted(os.path.basename(p)[len("model_train_"):-4] for p in glob.glob(os.path.join(GOLDEN, "model_train_*.npz")))


def load(name):
    d = np.load(os.path.join(GOLDEN, f"model_train_{name}.npz"))
    return json.loads(str(d["meta"])), d


def param_names(d, team):
    pre = f"init::{team}::"
    return [k[len(pre):] for k in d.files if k.startswith(pre)]


def step_indices(meta, d):
    idx, out = d["indices"].astype(np.int64), []
    off = 0
    for bs in meta["batch_sizes"]:
        out.append(idx[off:off + bs])
        off += bs
    return out


def check_first_step(d, team, exp_avg_by_name):
    """Gradients of the first step, recovered as exp_avg / (1 - beta1), within 1e-4 of each tensor's max-abs."""
    for n, got in exp_avg_by_name.items():
        key = f"first_exp_avg::{team}::{n}"
        if key not in d.files:
            assert float(np.abs(got).max()) == 0.0, f"{team} {n}: the reference took no first step"
            continue
        ref = d[key] / (1 - BETA1)
        g = got / (1 - BETA1)
        scale = max(float(np.abs(ref).max()), 1e-30)
        assert float(np.abs(g - ref).max()) <= 1e-4 * scale, f"{team} {n}: first-step gradient off by {float(np.abs(g - ref).max()) / scale:.2e}"


def check_final(d, team, params_by_name, step):
    """After K steps: ||p - p_ref|| / ||p_ref - p_init|| <= 1e-3 per tensor, and the Adam step count exact."""
    for n, p in params_by_name.items():
        ref, init = d[f"final::{team}::{n}"], d[f"init::{team}::{n}"]
        moved = float(np.linalg.norm(ref.astype(np.float64) - init))
        err = float(np.linalg.norm(p.astype(np.float64) - ref))
        assert err <= 1e-3 * moved or (moved == 0.0 and err == 0.0), f"{team} {n}: {err:.3e} vs moved {moved:.3e}"
        assert float(d[f"final_step::{team}::{n}"]) == float(step), f"{team} {n}: step {step} vs {float(d[f'final_step::{team}::{n}'])}"


def mlp_from(pkg, d, team, dims):
    m = pkg.MLP(dims)
    m.load_state_dict({n: torch.tensor(d[f"init::{team}::{n}"]) for n in param_names(d, team)})
    return m
