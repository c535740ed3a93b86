"""CPU-only checks of tests/spatial_train_walk.py: the grid's constants against the headers, the literal grid of every case and that the
case walks what it was chosen to walk, the batch builder's lists, the host-side workspace queries on every case's shapes -- and the three
conditions on the cases whose recurrence kernel walks, from the float64 and float32 torch references ALONE (the code under test is never
run here): the reference depends on the second pass's rows and on the last tile's far beyond the tolerance, and the float32 torch path
itself stays within a quarter of it.

Chosen inputs and their measured guards (exp_avg per parameter tensor, in units of the tensor's float64 max-abs; minimum over all tensors
of both teams and both layouts for the influences, maximum for the yardstick):
  rows         second pass x 10, its one-row last tile x 10 on top: second-pass influence 0.062, last-tile influence 0.025, yardstick 1.8e-6
  partial_cap  second pass x 3, last tile x 3 on top, lr 1e-4:      second-pass influence 0.17, last-tile influence 0.13, yardstick 6.2e-6
against the conditions 1e-2 (100 x the tolerance), 1e-3 (10 x) and 2.5e-5 (a quarter)."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import spatial_train_walk as W
from spatial_train_util import fill_net, make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sus-net_amd", "csrc")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_the_restated_constants_are_the_headers(pkg):
    text = lambda *p: open(os.path.join(*p)).read()
    assert int(re.search(r"#define SUSNET_SPATIAL_TRAIN_MAX_GRID (\d+)", text(ROOT, "include", "susnet.h")).group(1)) == pkg._lib.SPATIAL_TRAIN_MAX_GRID == 256
    assert int(re.search(r"constexpr int kStConvGrid = (\d+);", text(CSRC, "susnet_spatial_train.h")).group(1)) == W.CONV_GRID
    assert int(re.search(r"kMtMaxPartialBytes = (\d+)ull << 20;", text(CSRC, "susnet_mlp_train.h")).group(1)) << 20 == W.MAX_PARTIAL_BYTES
    assert int(re.search(r"kTrTS = (\d+)", text(CSRC, "susnet_train_core.h")).group(1)) == W.TILE


@pytest.mark.parametrize("name", list(W.CASES))
def test_every_case_has_its_literal_grid_and_walks_what_it_names(pkg, name):
    c = W.CASES[name]
    G, Gconv, tiles, images = grid = W.case_grid(name)
    assert grid == c.grid, (name, grid, c.grid)
    assert c.T >= 2, "with T = 1 the W_hh gradient is identically zero: no guard can hold on it"
    models, targets = W.case_models(name)
    rnn = [m.rnn.model for m in models]
    if name == "rows":
        assert (G, tiles) == (256, 385) and tiles - G == 129 and c.n - (tiles - 1) * W.TILE == 1  # workgroups 0 .. 128, the last tile one row
        assert images // G == 96 and 2 * images // Gconv == 48
        assert [r.num_layers for r in rnn] == [2, 1] and [r.hidden_size for r in rnn] == [9, 5]
    if name == "partial_cap":
        assert (G, tiles) == (15, 17) and c.n - (tiles - 1) * W.TILE == 1
        assert max(W.n_params(m) for m in models) == 1115921 and G == W.MAX_PARTIAL_BYTES // (4 * 1115924)
        assert all(r.input_size == pkg._lib.SPATIAL_MAX_R == 4096 and r.hidden_size == 256 for r in rnn)
    if name == "images":
        assert tiles <= G < images and 2 * images <= Gconv, "conv_bwd walks, the recurrence and conv do not"
        assert [r.num_layers for r in rnn] == [3, 4] and [r.hidden_size for r in rnn] == [129, 256] and c.T == pkg._lib.SPATIAL_MAX_T
    if name == "jobs":
        assert 2 * images == 1040 > Gconv == 1024 and tiles <= G
    if name == "wide_image":
        assert rnn[0].input_size == 4096 and c.Fn == 0 and c.N == 16 and tiles <= G
        assert len([m for m in models[1].cnn.model if isinstance(m, torch.nn.Conv2d)]) == 3  # (the target's ping-pong has two halves in use)
    assert len(W.second_pass_rows(name)) == max(0, c.n - W.TILE * G)
    for a, b in zip(models, targets):
        assert not torch.equal(next(a.parameters()), next(b.parameters())), "the target network has weights of its own"


@pytest.mark.parametrize("name", list(W.DROPOUT_GRIDS))
def test_the_dropout_networks_still_walk(name):
    c = W.CASES[name]
    models, _ = W.dropout_models(name)
    grid = W.documented_grid(models, c.n, c.T)
    assert grid == W.DROPOUT_GRIDS[name] and grid[2] > grid[0], (name, grid)
    assert all(m.rnn.model.num_layers >= 2 and m.rnn.model.dropout == 0.2 for m in models), "a second layer: the multipliers' slice exists"


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_batch_puts_every_position_into_three_lists(name):
    """The lists restated: list (agent, imposter team) = the batch positions s, ascending, with imposters[idx[s]] == agent; the crew list
    the others.  Second-pass and last-tile rows carry their factors, negation flips exactly those rows, the layouts share everything else."""
    c = W.CASES[name]
    b = W.walk_batch(name)
    assert np.array_equal(b["idx"], np.arange(c.n)) and len(b["rewards"]) == c.n == len(b["imposters"])
    who = b["imposters"][b["idx"]]
    lists = {(agent, team): np.flatnonzero((who == agent) == (team == 0)) for agent in range(W.A3) for team in range(2)}
    for key, rows in lists.items():
        assert len(rows) == (c.n if key in ((0, 0), (1, 1), (2, 1)) else 0), key
        assert np.array_equal(rows, np.arange(len(rows)))  # position p of the list is batch position p: tile p // 32
    base = make_batch(np.random.default_rng(1000 * c.seed), c.n, c.T, W.A3, c.C, c.N, c.Fn, 4, M=c.n, density=c.density)  # (the rewards before the factors)
    G = W.case_grid(name)[0]
    want = base["rewards"].copy()
    want[W.TILE * G:] *= np.float32(c.factor)
    want[(c.n - 1) // W.TILE * W.TILE:] *= np.float32(c.last_factor)
    assert np.array_equal(b["rewards"], want) and b["rewards"].dtype == np.float32
    for which, rows in (("second_pass", W.second_pass_rows(name)), ("last_tile", W.last_tile_rows(name))):
        flipped = W.walk_batch(name, negate=which)
        sign = np.ones(c.n, dtype=np.float32)
        sign[rows] = -1.0
        assert np.array_equal(flipped["rewards"], b["rewards"] * sign[:, None])
        assert all(np.array_equal(flipped[k], b[k]) for k in b if k != "rewards")
    g = W.walk_batch(name, "global")
    assert g["spatial"].shape == (c.n, c.T, c.C, c.N, c.N) and np.array_equal(g["spatial"], b["spatial"][:, :, 0])
    assert all(np.array_equal(g[k], b[k]) for k in b if "spatial" not in k or "non" in k)
    other = W.walk_batch(name, seed_shift=1)
    assert not np.array_equal(other["spatial"], b["spatial"]) and not np.array_equal(other["rewards"], b["rewards"])


def _io(pkg, models, c, layout):
    """A susnet_spatial_train_io of the case's shapes with plausible, never dereferenced pointers (the queries read shapes only)."""
    L = pkg._lib
    io = L.SpatialTrainIO()
    for field in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        setattr(io, field, 4096)
    io.max_size, io.n, io.gamma = c.n, c.n, W.GAMMA
    img = c.C * c.N * c.N
    strides = (c.T * W.A3 * img, img, W.A3 * img) if layout == "perspective" else (c.T * img, 0, img)
    for d in range(3):
        io.spatial_stride[d], io.non_spatial_stride[d] = strides[d], (c.T * W.A3 * c.Fn, c.Fn, W.A3 * c.Fn)[d]
    for t, m in enumerate(models):
        tm = io.team[t]
        dims = [m.rnn.model.hidden_size] + [l.out_features for l in m.prediction_head if isinstance(l, torch.nn.Linear)]
        tm.enabled, tm.n_dims = 1, len(dims)
        for k, d in enumerate(dims):
            tm.dims[k] = d
        tm.lr, tm.beta1, tm.beta2, tm.eps = c.lr, 0.9, 0.999, 1e-8
        tm.params = tm.target_params = tm.exp_avg = tm.exp_avg_sq = tm.step = 4096
        fill_net(io.net[t], m, c.T)
    return io


@pytest.mark.parametrize("layout", ["perspective", "global"])
@pytest.mark.parametrize("name", list(W.CASES))
def test_the_workspace_queries_accept_every_case(pkg, name, layout):
    """susnet_spatial_train_workspace_bytes and its dropout twin on a handle without device buffers (3 agents, one imposter): accepted, and
    the sizes hold at least what the documented grid implies -- G partials of Pp floats, and under dropout G slices of multipliers on top."""
    L = pkg._lib
    lib = L.lib()
    h = W.host_handle(L, lib)
    c = W.CASES[name]
    nbytes, dbytes = C.c_uint64(), C.c_uint64()
    for models in [W.case_models(name)[0]] + ([W.dropout_models(name)[0]] if name in W.DROPOUT_GRIDS else []):
        io = _io(pkg, models, c, layout)
        assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(io), C.byref(nbytes)) == 0, (name, lib.susnet_last_error())
        assert lib.susnet_spatial_train_dropout_workspace_bytes(h, C.byref(io), C.byref(dbytes)) == 0, (name, lib.susnet_last_error())
        G = W.documented_grid(models, c.n, c.T)[0]
        pp = max((W.n_params(m) + 1 + 3) // 4 * 4 for m in models)
        assert nbytes.value % 256 == 0 and nbytes.value >= 4 * G * pp
        mslice = max((m.rnn.model.num_layers - 1) * c.T * m.rnn.model.hidden_size * W.TILE for m in models)
        assert dbytes.value - nbytes.value == (4 * G * max(mslice, 4) + 255) // 256 * 256, (name, dbytes.value, nbytes.value, G, mslice)
    lib.susnet_destroy(h)


@pytest.mark.parametrize("layout", ["perspective", "global"])
@pytest.mark.parametrize("name", W.GUARDED)
def test_the_three_conditions_on_the_walking_cases(name, layout):
    """Second-pass influence >= 1e-2, last-tile influence >= 1e-3 and the float32 yardstick <= 2.5e-5 of each tensor's float64 max-abs, on
    EVERY parameter tensor of both teams: a step that drops, repeats or overwrites a second pass cannot stay within 1e-4."""
    second, last, yard = W.influence(name, "second_pass", layout), W.influence(name, "last_tile", layout), W.yardstick(name, layout)
    for t in range(2):
        for tensor in yard[t]:
            print(f"{name} {layout} team {t} {tensor}: second pass {second[t][tensor]:.2e}, last tile {last[t][tensor]:.2e}, float32 torch {yard[t][tensor]:.2e}")
    for t in range(2):
        for tensor in yard[t]:
            assert second[t][tensor] >= W.SECOND_PASS_MIN, (t, tensor, second[t][tensor])
            assert last[t][tensor] >= W.LAST_TILE_MIN, (t, tensor, last[t][tensor])
            assert yard[t][tensor] <= W.YARDSTICK_MAX, (t, tensor, yard[t][tensor])
    _, _, counts = W.reference(name, layout)
    assert counts == [1.0, 2.0]  # one imposter update (agent 0), two crew updates (agents 1 and 2)
