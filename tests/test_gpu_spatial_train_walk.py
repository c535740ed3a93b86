"""The SpatialDQN train step (susnet_spatial_train_step, its dropout form and its sweep) on the MI355X where a workgroup does MORE THAN ONE
unit of work: k_sp_train_rnn walking a second tile (every `first ? acc : *w + acc` on its second side, the slices, `rid` and the LDS buffers
reused), k_sp_train_conv_bwd owning several images, k_sp_train_conv grid-striding over jobs -- and hidden 256 (all 8 waves carry a unit
block), R = 4096 and Rc = 4096.  tests/spatial_train_walk.py has the cases, tests/test_spatial_train_walk_host.py shows without a GPU that
every case has the grid it was chosen for and that the float64 reference of the walking cases depends on the second pass's rows by at
least 100 x the tolerance.  The criteria are the project's for this step, unchanged: Adam step counts exact, losses rtol 1e-4 of float64,
every parameter tensor's exp_avg within 1e-4 of its float64 max-abs, canaries and the workspace guard intact.

Every comparison prints the kernel's error beside the float32 torch path's own (run with -s); DESIGN.md 7a records the figures."""
import importlib

import numpy as np
import pytest
import torch

import spatial_train_walk as W
from spatial_dropout_util import library_masks, masked_reference
from spatial_sweep_util import SweepCall, dropout_step, dropout_workspace, make_drop, same_bits
from spatial_train_util import SpatialCall, compare_tensors
from train_exact import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env3(pkg):
    """A 3-agent, one-imposter handle (test_gpu_spatial_train.py's): the step takes the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


def _check(models, losses, got, l64, ea64, st64, l32, ea32, what):
    for t in range(2):
        assert got[t]["step"] == st64[t] == (1.0, 2.0)[t], (t, got[t]["step"], st64[t])
        compare_tensors(models[t], got[t]["exp_avg"], ea64[t], ea32[t], f"{what} team {t}", tol=W.TOL)
    print(f"{what} losses: kernel rel {np.abs(losses - l64) / np.abs(l64)}, float32 torch rel {np.abs(l32 - l64) / np.abs(l64)}")
    np.testing.assert_allclose(losses, l64, rtol=W.TOL)


# ---- 1. every case against float64, both layouts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["global", "perspective"])
@pytest.mark.parametrize("name", list(W.CASES))
def test_walk_against_float64(pkg, env3, name, layout):
    """One call on the case's batch against torch_train_step on float64 CPU copies (the float32 torch path's own error printed beside the
    kernel's).  The grid is asserted first: the case walks what its row of the table says."""
    assert W.case_grid(name) == W.CASES[name].grid
    models, targets = W.case_models(name)
    l64, ea64, st64 = W.reference(name, layout)
    l32, ea32, _ = W.reference(name, layout, "float32")
    losses, got = SpatialCall(pkg, env3, models, targets, W.walk_batch(name, layout), W.GAMMA, lr=W.CASES[name].lr).step()
    _check(models, losses, got, l64, ea64, st64, l32, ea32, f"{name} {layout}")


# ---- 2. the dropout form: a second tile's multipliers are those of its own rows ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.DROPOUT_GRIDS))
def test_dropout_walk_against_float64(pkg, env3, name):
    """susnet_spatial_train_step_dropout with at least two RNN layers per team (the multipliers' slice msl exists and is rewritten per tile)
    against masked_train_step in float64 under the library's own exported masks, online p = 0.2 and target p = 0.5; the same restatement in
    float32 gives the error printed beside the kernel's."""
    c = W.CASES[name]
    models, targets = W.dropout_models(name)
    assert W.documented_grid(models, c.n, c.T) == W.DROPOUT_GRIDS[name]
    batch = W.walk_batch(name)
    drops = make_drop(pkg, 0.2, 0.5, seed=1, offset=3)
    masks = library_masks(pkg, env3, models, drops, c.n, c.T, W.A3)
    l64, ea64, st64 = masked_reference(models, targets, batch, W.GAMMA, c.lr, masks)
    l32, ea32, _ = masked_reference(models, targets, batch, W.GAMMA, c.lr, masks, torch.float32)
    call = dropout_workspace(pkg, env3, SpatialCall(pkg, env3, models, targets, batch, W.GAMMA, lr=c.lr))
    losses, got = dropout_step(pkg, env3, call, drops)
    _check(models, losses, got, l64, ea64, st64, l32, ea32, f"{name} dropout")


# ---- 3. the sweep forms: every learner bitwise its own single call ---------------------------------------------------------------------------------
def _learners(pkg, env3, name, models_of):
    """K = 2 learners on DIFFERENT batches with different gamma and lr, built twice: the sweep's calls and their twins."""
    models, targets = models_of(name)
    return [[SpatialCall(pkg, env3, models, targets, W.walk_batch(name, seed_shift=k), (0.9, 0.8)[k], lr=(1e-3, 3e-3)[k]) for k in range(2)] for _ in range(2)]


@pytest.mark.parametrize("name", list(W.DROPOUT_GRIDS))
def test_sweep_walk_is_bitwise_the_single_step(pkg, env3, name):
    calls, twins = _learners(pkg, env3, name, W.case_models)
    got = SweepCall(pkg, env3, calls).step()
    for k, twin in enumerate(twins):
        same_bits(got[k], twin.step(), f"{name} learner {k}")
    assert not np.array_equal(got[0][1][0]["bits"][1], got[1][1][0]["bits"][1]), "the learners are different learners"


@pytest.mark.parametrize("name", list(W.DROPOUT_GRIDS))
def test_dropout_sweep_walk_is_bitwise_the_dropout_step(pkg, env3, name):
    """Learner 0 under online and target masks, learner 1 under online masks only (the library refuses a sweep in which one learner's team
    is masked and another's is not: every learner has a p > 0)."""
    calls, twins = _learners(pkg, env3, name, W.dropout_models)
    for c in calls + twins:
        dropout_workspace(pkg, env3, c)
    drops = [make_drop(pkg, 0.2, 0.5, seed=11, offset=3), make_drop(pkg, 0.5, 0.0, seed=(1 << 40) + 7, offset=(1 << 33) + 1)]
    got = SweepCall(pkg, env3, calls, drops).step()
    for k, twin in enumerate(twins):
        same_bits(got[k], dropout_step(pkg, env3, twin, drops[k]), f"{name} learner {k}")


# ---- 4. reproducible, capturable --------------------------------------------------------------------------------------------------------------
def test_two_runs_of_rows_leave_identical_bytes(pkg, env3):
    models, targets = W.case_models("rows")
    runs = []
    for _ in range(2):
        call = SpatialCall(pkg, env3, models, targets, W.walk_batch("rows"), W.GAMMA, lr=W.LR)
        call.step()
        runs.append(call.step())
    same_bits(runs[0], runs[1], "rows, two runs")


def test_graph_replay_of_rows_matches_eager(pkg, env3):
    """One captured call replayed (single stream, as test_gpu_spatial_train.test_graph_replay_matches_eager captures) equals the eager call."""
    models, targets = W.case_models("rows")
    batch = W.walk_batch("rows")
    eager = SpatialCall(pkg, env3, models, targets, batch, W.GAMMA, lr=W.LR)
    want = [eager.step() for _ in range(2)]
    call = SpatialCall(pkg, env3, models, targets, batch, W.GAMMA, lr=W.LR)
    call.step()  # one eager step first: kernel attributes (step 1 of 2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    state = [g[k].buf for g in call.bufs for k in ("params", "exp_avg", "exp_avg_sq")] + [g["step"] for g in call.bufs]
    saved = [x.clone() for x in state]
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call.launch()
    torch.cuda.current_stream().wait_stream(s)
    for x, sv in zip(state, saved):  # (capturing runs nothing; restore in case the runtime did)
        x.copy_(sv)
    graph.replay()
    torch.cuda.synchronize()
    same_bits(call.results(), want[1], "rows, replay")
