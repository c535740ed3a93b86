"""CPU checks of the train step's host side: the C structs of susnet_dqn_train_step against their ctypes mirror, and the torch
path's semantics of DQNTeamTrainer.train_step (src/train.py:50-149): gradients accumulate over agents, empty teams take no step."""
import copy
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_dqn_structs_match_ctypes(pkg, tmp_path):
    L = pkg._lib
    structs = {"susnet_dqn_team": L.DqnTeam, "susnet_dqn_io": L.DqnIO}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){"]
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ["return 0;}"]
    prog = tmp_path / "dqn_sizes.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "dqn_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, ct in structs.items():
        assert int(out[name]) == C.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(ct, fname).offset, f"{name}.{fname}"
    assert {"susnet_dqn_train_step", "susnet_dqn_workspace_bytes"} <= set(L.EXPORTS)


def _batch(A=3, N=12, F_=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = (torch.rand(N, 1, F_, generator=g) > 0.5).float()
    nfeats = (torch.rand(N, 1, F_, generator=g) > 0.5).float()
    actions = torch.randint(0, 4, (N, A), generator=g)
    rewards = torch.randn(N, A, generator=g)
    dones = torch.rand(N, 1, generator=g) > 0.7
    imposters = torch.randint(0, A, (N, 1), generator=g).to(torch.int16)
    z = torch.zeros(N, 1, 1)
    return [(z, feats)] * A, [(z, nfeats)] * A, actions, rewards, dones, imposters


def _net(pkg, seed, F_=10, n_out=4):
    torch.manual_seed(seed)
    return pkg.MLP([F_, 8, 8, 8, 8, n_out])


def test_torch_path_accumulates_gradients_like_the_reference(pkg):
    sf, nf, actions, rewards, dones, imposters = _batch()
    imp, crew = _net(pkg, 1), _net(pkg, 2)
    timp, tcrew = imp.create_copy(), crew.create_copy()
    oi, oc = torch.optim.Adam(imp.parameters(), lr=1e-2), torch.optim.Adam(crew.parameters(), lr=1e-2)
    # restated by hand: zero_grad once, then per agent (imposter, crew) backward + step, the .grad accumulating
    imp2, crew2 = copy.deepcopy(imp), copy.deepcopy(crew)
    oi2, oc2 = torch.optim.Adam(imp2.parameters(), lr=1e-2), torch.optim.Adam(crew2.parameters(), lr=1e-2)
    expect = [0.0, 0.0]
    oi2.zero_grad()
    oc2.zero_grad()
    for a in range(3):
        m = (imposters == a).view(-1)
        for team, rows, mod, tgt, opt in ((0, m, imp2, timp, oi2), (1, ~m, crew2, tcrew, oc2)):
            if int(rows.sum()) == 0:
                continue
            q = mod(sf[a][0][rows], sf[a][1][rows]).gather(1, actions[rows, a].view(-1, 1)).view(-1)
            with torch.no_grad():
                r = rewards[rows, a]
                y = r + 0.9 * tgt(nf[a][0][rows], nf[a][1][rows]).max(dim=1)[0]
                y[dones[rows].view(-1)] = r[dones[rows].view(-1)]
            loss = F.mse_loss(q, y)
            loss.backward()
            expect[team] += loss.item()
            opt.step()
    got = pkg.torch_train_step([imp, crew], [timp, tcrew], [oi, oc], 0.9, sf, nf, actions, rewards, dones, imposters)
    assert got == pytest.approx(expect, rel=1e-6)
    for p, q in zip(list(imp.parameters()) + list(crew.parameters()), list(imp2.parameters()) + list(crew2.parameters())):
        assert torch.equal(p, q)


def test_torch_path_skips_empty_teams(pkg):
    sf, nf, actions, rewards, dones, imposters = _batch(N=4)
    imposters[:] = 0  # agent 0 is the imposter everywhere: agents 1, 2 have no imposter rows, agent 0 no crew rows
    imp, crew = _net(pkg, 1), _net(pkg, 2)
    oi, oc = torch.optim.Adam(imp.parameters(), lr=1e-2), torch.optim.Adam(crew.parameters(), lr=1e-2)
    pkg.torch_train_step([imp, crew], [imp.create_copy(), crew.create_copy()], [oi, oc], 0.9, sf, nf, actions, rewards, dones, imposters)
    step = lambda o: float(next(iter(o.state.values()))["step"])
    assert step(oi) == 1 and step(oc) == 2


def test_two_imposters_are_refused(pkg):
    sf, nf, actions, rewards, dones, _ = _batch(N=4)
    imp = _net(pkg, 1)
    with pytest.raises(ValueError, match="train.py:83"):
        pkg.torch_train_step([imp, None], [imp.create_copy(), None], [torch.optim.Adam(imp.parameters()), None], 0.9, sf, nf, actions, rewards,
                             dones, torch.zeros(4, 2, dtype=torch.int16))


# ---- the torch path against the reference's own train_step (tests/golden/model_train_*.npz, generate_train.py) ----
from train_fixtures import check_final, check_first_step, fixture_names, load, mlp_from, param_names, step_indices  # noqa: E402


@pytest.mark.parametrize("name", fixture_names())
def test_torch_path_reproduces_reference_fixture(pkg, name):
    meta, d = load(name)
    A = meta["n_agents"]
    models = [mlp_from(pkg, d, "imposter", meta["imposter_dims"]), mlp_from(pkg, d, "crew", meta["crew_dims"])]
    targets = [m.create_copy() for m in models]
    trained = [meta["train_imposter"], meta["train_crew"]]
    opts = [torch.optim.Adam(m.parameters(), lr=meta["lr"]) if tr else None for m, tr in zip(models, trained)]
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
                if opts[t] is not None:
                    names = dict(models[t].named_parameters())
                    check_first_step(d, team, {n: (opts[t].state[names[n]]["exp_avg"].numpy() if names[n] in opts[t].state else np.zeros(names[n].shape))
                                               for n in param_names(d, team)})
    for t, team in enumerate(("imposter", "crew")):
        names = dict(models[t].named_parameters())
        step = 0.0
        if opts[t] is not None and opts[t].state:
            step = float(next(iter(opts[t].state.values()))["step"])
        check_final(d, team, {n: names[n].detach().numpy() for n in param_names(d, team)}, step)


def test_fixtures_exercise_dones_and_skips():
    names = fixture_names()
    assert {"itg_1v1_onehot", "itg_1v1_walls_coord", "base14_1v2_j4"} <= set(names)
    meta, d = load("itg_1v1_onehot")
    assert meta["done_rows"] > 0
    meta, d = load("base14_1v2_j4")
    assert len(set(d["ring::imposters"].reshape(-1).tolist())) == 3 and min(meta["batch_sizes"]) == 1
