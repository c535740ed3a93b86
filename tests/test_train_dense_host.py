"""The package's torch path (``torch_train_step``) against the reference's own train_step on a game and on layer stacks the compiled-in
layouts do not know: tests/golden/dense/dense_train_*.npz (generate_train_dense.py: base 9x9 1v3 with 5 jobs; hidden (48, 24) on onehot_pos +
alive_crew + closest_crew, hidden (40, 33, 20, 12, 9, 8) on coord_pos + alive_crew).  This pins the yardstick the dense HIP step
(tests/test_gpu_mlp_train.py) is measured with; no GPU is needed."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from train_fixtures import GOLDEN, check_final, check_first_step, mlp_from, param_names, step_indices

NAMES = ["base9_1v3_j5_comps3", "base9_1v3_j5_coord_deep"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def load_dense(name):
    d = np.load(os.path.join(GOLDEN, "dense", f"dense_train_{name}.npz"))
    return json.loads(str(d["meta"])), d


@pytest.mark.parametrize("name", NAMES)
def test_torch_path_reproduces_dense_reference_fixture(pkg, name):
    meta, d = load_dense(name)
    A = meta["n_agents"]
    models = [mlp_from(pkg, d, "imposter", meta["imposter_dims"]), mlp_from(pkg, d, "crew", meta["crew_dims"])]
    targets = [m.create_copy() for m in models]
    opts = [torch.optim.Adam(m.parameters(), lr=meta["lr"]) for m in models]
    fs = torch.tensor(d["feat_states"], dtype=torch.float32).unsqueeze(1)
    fn = torch.tensor(d["feat_next_states"], dtype=torch.float32).unsqueeze(1)
    ring = {k: torch.tensor(d["ring::" + k]) for k in ("actions", "rewards", "dones", "imposters")}
    for k, idx in enumerate(step_indices(meta, d)):
        i = torch.tensor(idx)
        z = torch.zeros(len(idx), 1, 1)
        losses = pkg.torch_train_step(models, targets, opts, meta["gamma"], [(z, fs[i])] * A, [(z, fn[i])] * A, ring["actions"][i].long(),
                                      ring["rewards"][i].float(), ring["dones"][i].bool().reshape(-1, 1), ring["imposters"][i].to(torch.int16))
        np.testing.assert_allclose(losses, d["losses"][k], rtol=1e-4, atol=1e-7)
        if k == 0:
            for t, team in enumerate(("imposter", "crew")):
                names = dict(models[t].named_parameters())
                check_first_step(d, team, {n: (opts[t].state[names[n]]["exp_avg"].numpy() if names[n] in opts[t].state else np.zeros(names[n].shape))
                                           for n in param_names(d, team)})
    for t, team in enumerate(("imposter", "crew")):
        names = dict(models[t].named_parameters())
        step = float(next(iter(opts[t].state.values()))["step"]) if opts[t].state else 0.0
        check_final(d, team, {n: names[n].detach().numpy() for n in param_names(d, team)}, step)


def test_dense_fixtures_are_what_the_tests_need():
    for name, hidden in zip(NAMES, ([48, 24], [40, 33, 20, 12, 9, 8])):
        meta, d = load_dense(name)
        assert meta["hidden"] == hidden and meta["n_agents"] == 4 and meta["n_imposters"] == 1 and meta["kwargs"]["n_jobs"] == 5
        assert meta["done_rows"] >= 8 and meta["dones_set_every"] == 8 and int(d["ring::dones"].sum()) == meta["done_rows"]
        assert d["ring::states"].shape[0] == 256 and sorted(set(meta["batch_sizes"])) == [1, 3, 32] and len(meta["batch_sizes"]) == 12
        assert len(set(d["ring::imposters"].reshape(-1).tolist())) >= 2  # shuffled imposter index: more than one agent is the imposter
        assert os.path.getsize(os.path.join(GOLDEN, "dense", f"dense_train_{name}.npz")) < 256 * 1024
    # the compiled-in layouts do not know these: F is neither 36, 4 nor 88, and the stacks are not five Linear layers
    assert load_dense(NAMES[0])[0]["imposter_dims"][0] == 4 * 18 + 3 + 3 and load_dense(NAMES[1])[0]["imposter_dims"][0] == 8 + 3
