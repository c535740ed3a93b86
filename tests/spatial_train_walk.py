"""Shared by the tests of the SpatialDQN train step at the sizes where a workgroup does MORE THAN ONE unit of work (a second tile of 32 list
rows in k_sp_train_rnn, several images in k_sp_train_conv_bwd, a second job in k_sp_train_conv): the case table, the grid's documented
formula restated, the batch builder whose lists hold every batch position, and the guards that say a case's float64 reference DEPENDS on
the rows a workgroup meets on its second pass.  Importing this module touches no GPU, and nothing in it runs the code under test: the
references are spatial_train_util.torch_reference on CPU copies, computed once per (case, layout, variant) and shared."""
import ctypes
import functools
import importlib
from collections import namedtuple

import numpy as np
import torch

from spatial_train_util import as_global, make_batch, make_model, split, torch_reference

A3 = 3                              # 1 imposter + 2 crew: the env3 handle of test_gpu_spatial_train.py
TILE = 32                           # kTrTS: list rows of a tile of k_sp_train_rnn
MAX_PARTIAL_BYTES = 64 << 20        # kMtMaxPartialBytes (csrc/susnet_mlp_train.h): all workgroups' partials together
CONV_GRID = 1024                    # kStConvGrid (csrc/susnet_spatial_train.h): workgroups of k_sp_train_conv
GAMMA, LR = 0.9, 1e-3
TOL = 1e-4                          # the project's criterion: exp_avg per tensor within TOL of the tensor's float64 max-abs, losses rtol TOL
SECOND_PASS_MIN, LAST_TILE_MIN, YARDSTICK_MAX = 100 * TOL, 10 * TOL, TOL / 4

# a network: (chans behind C, k, strides, pads, dils, rnn layers, hidden, head hidden widths), as test_gpu_spatial_train.RAGGED has them
Case = namedtuple("Case", "n T N C Fn imposter crew grid factor last_factor density seed what lr", defaults=(LR,))

# `grid`: the literal (G, Gconv, tiles, images) the case was chosen for -- asserted beside the restated formula, so a change of the library's
# formula fails the case instead of silently no longer walking.  `factor` multiplies the rewards of the rows of a workgroup's SECOND pass
# (list positions >= 32 G), `last_factor` those of the last tile's rows on top of it (test_spatial_train_walk_host.py has the measured guards).
SMALL = ([3], 3, [1], [1], [1], 2, 7, [6])  # test_gpu_spatial_train._small()
CASES = {
    # 385 tiles against 256 workgroups: workgroups 0 .. 128 walk two tiles, the last tile (workgroup 128's second) has ONE row; 24 578 images,
    # 96 or 97 per workgroup of conv_bwd; 49 156 conv jobs, 48 or 49 per workgroup
    "rows": Case(12289, 2, 5, 3, 2, ([2], 3, [1], [1], [1], 2, 9, [6]), ([], 1, [1], [0], [1], 1, 5, []), (256, 1024, 385, 24578), 10.0, 10.0, 0.3, 7,
                 "k_sp_train_rnn walks a second tile (one of them a 1-row tile), conv_bwd 96 images and conv 48 jobs per workgroup"),
    # P = 1 115 921 (imposters): 64 MiB of partials allow 15 workgroups against 17 tiles -- workgroup 0 walks a second full tile (15),
    # workgroup 1 the 1-row last tile (16).  R = 4096 and H = 256 are the limits.  Factor 3 and lr = 1e-4 keep the float32 torch path
    # itself within 6e-6 of float64: the crew's second update starts from parameters Adam moved by about lr whatever the gradient's size, so
    # float32 rounding in the first update reaches the second amplified by lr
    "partial_cap": Case(513, 2, 5, 3, 4096 - 75, ([], 1, [1], [0], [1], 1, 256, []), ([], 1, [1], [0], [1], 1, 256, []), (15, 1024, 17, 1026), 3.0, 3.0,
                        0.3, 6, "the 64 MiB cap shrinks G below the tiles; R = 4096, H = 256: all 8 waves carry a unit block", 1e-4),
    # two tiles, no tile walk; G = 34 (ONE grid per call, from the wider team: the crew's P = 481 552; the imposters' 108 504 alone would give
    # 154): 320 images, 9 or 10 per workgroup of conv_bwd; conv (640 jobs against 1024) does not walk.  L, T, H at the limits
    "images": Case(40, 8, 5, 3, 2, ([2], 3, [1], [1], [1], 3, 129, [130, 6]), ([], 1, [1], [0], [1], 4, 256, []), (34, 640, 2, 320), 1.0, 1.0, 0.3, 3,
                   "k_sp_train_conv_bwd owns several images and nothing else walks; rnn layers 4, T 8, hidden 256 are the limits"),
    # 1040 conv jobs against 1024 workgroups: 16 workgroups reuse their target ping-pong slice
    "jobs": Case(65, 8, 5, 3, 2, SMALL, SMALL, (256, 1024, 3, 520), 1.0, 1.0, 0.3, 4, "k_sp_train_conv grid-strides with the least else"),
    # Rc = R = 16 x 16 x 16 = 4096: dX over 128 column blocks, conv_bwd on 16 x 16 images with 16 channels (G = 62: the imposters' P = 269 846)
    "wide_image": Case(40, 2, 16, 4, 0, ([16], 3, [1], [1], [1], 1, 64, [8]), ([8, 8], 3, [2, 1], [1, 1], [1, 1], 2, 33, []), (62, 160, 2, 80), 1.0, 1.0,
                       0.3, 5, "dX over Rc = 4096 columns; the widest image the convolutions' backward serves"),
}
GUARDED = ("rows", "partial_cap")  # the cases whose k_sp_train_rnn walks: the three conditions are checked on these


def _pkg():
    return importlib.import_module("sus-net_amd")


def host_handle(L, lib):
    """A 3-agent, one-imposter handle without device buffers, as tests/test_spatial_train_abi.py makes its own: enough for the workspace queries."""
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = ctypes.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=8, n_imposters=1, n_crew=A3 - 1, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                     shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = ctypes.c_void_p()
    assert lib.susnet_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.susnet_last_error()
    return h


def n_params(model):
    return sum(p.numel() for p in model.parameters())


def documented_grid(models, n, T):
    """G = max(1, min(SUSNET_SPATIAL_TRAIN_MAX_GRID, n T, 64 MiB / (4 Pp))) workgroups of k_sp_train_rnn and k_sp_train_conv_bwd (Pp: the widest
    enabled team's P + 1, rounded up to 4), Gconv = min(1024, 2 n T) of k_sp_train_conv -- susnet_spatial_train.h's formula, restated;
    -> (G, Gconv, tiles of 32 rows in a list of n, images of such a list)."""
    max_grid = _pkg()._lib.SPATIAL_TRAIN_MAX_GRID
    pp = max((n_params(m) + 1 + 3) // 4 * 4 for m in models if m is not None)
    images = max(1, n * T)
    return max(1, min(max_grid, images, MAX_PARTIAL_BYTES // (4 * pp))), min(CONV_GRID, 2 * images), (n + TILE - 1) // TILE, n * T


@functools.lru_cache(maxsize=None)
def case_models(name):
    """([imposter, crew], their targets -- other weights, so a kernel that reads the wrong one of the two is seen).  Not to be modified."""
    c = CASES[name]
    mk = lambda seed: [make_model(_pkg(), c.N, c.C, c.Fn, spec[0], spec[2], spec[3], spec[1], spec[4], spec[5], spec[6], spec[7], (5, 4)[t],
                                  seed + t) for t, spec in enumerate((c.imposter, c.crew))]
    return mk(100 * c.seed), mk(100 * c.seed + 50)


DROPOUT_GRIDS = {"rows": (256, 1024, 385, 24578), "partial_cap": (13, 1024, 17, 1026)}  # the literal grids of dropout_models: both still walk


@functools.lru_cache(maxsize=None)
def dropout_models(name, p=0.2):
    """The case's networks with AT LEAST TWO RNN layers and dropout p between them (both teams: every update is masked), and their targets --
    the networks of the dropout form on the case's batch.  On partial_cap the second layer's 131 584 parameters bring G from 15 to 13."""
    c = CASES[name]
    mk = lambda seed: [make_model(_pkg(), c.N, c.C, c.Fn, spec[0], spec[2], spec[3], spec[1], spec[4], max(2, spec[5]), spec[6], spec[7], (5, 4)[t],
                                  seed + t, dropout=p) for t, spec in enumerate((c.imposter, c.crew))]
    return mk(100 * c.seed + 7), mk(100 * c.seed + 57)


def case_grid(name):
    c = CASES[name]
    return documented_grid(case_models(name)[0], c.n, c.T)


def second_pass_rows(name):
    """List positions a workgroup meets on a pass after its first: p >= 32 G (position p lies in tile p // 32, walked by workgroup (p // 32) mod G)."""
    c = CASES[name]
    return np.arange(min(c.n, TILE * case_grid(name)[0]), c.n)


def last_tile_rows(name):
    c = CASES[name]
    return np.arange((c.n - 1) // TILE * TILE, c.n)


def walk_batch(name, layout="perspective", negate=None, seed_shift=0):
    """The case's batch: idx = arange(n) on a ring of n rows whose imposter is always agent 0 -- so agent 0's imposter list and the crew
    lists of agents 1 and 2 each hold ALL n batch positions in ascending order (tr_select<true>, susnet_train_core.h: every thread takes a
    contiguous ascending chunk and the chunks are placed in thread order), and the three other lists are empty.  The rewards of the second
    pass's rows are multiplied by the case's factor, the last tile's by its own on top.  ``negate``: "second_pass" / "last_tile" flips
    the sign of those rows' rewards (the influence guards)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c.seed + seed_shift)
    batch = make_batch(rng, c.n, c.T, A3, c.C, c.N, c.Fn, 4, M=c.n, density=c.density)
    batch["idx"] = np.arange(c.n, dtype=np.int64)
    batch["imposters"][:] = 0
    second, last = second_pass_rows(name), last_tile_rows(name)
    batch["rewards"][second] *= np.float32(c.factor)
    batch["rewards"][last] *= np.float32(c.last_factor)
    if negate is not None:
        batch["rewards"][{"second_pass": second, "last_tile": last}[negate]] *= np.float32(-1.0)
    return as_global(batch) if layout == "global" else batch


@functools.lru_cache(maxsize=None)
def reference(name, layout="perspective", dtype="float64", negate=None):
    """torch_reference of the case on CPU copies: (losses [2], exp_avg per team as flat float64, Adam step counts).  Shared: not to be modified."""
    models, targets = case_models(name)
    losses, ea, counts, _ = torch_reference(_pkg(), models, targets, walk_batch(name, layout, negate), GAMMA, CASES[name].lr, getattr(torch, dtype))
    return losses[0], ea, counts


def tensor_distances(model, a, b, ref):
    """{tensor name: max |a - b| over the tensor / the tensor's max-abs in ref}: the unit of compare_tensors' criterion."""
    out = {}
    for (name, x), (_, y), (_, r) in zip(split(model, a), split(model, b), split(model, ref)):
        out[name] = float(np.abs(x - y).max()) / max(float(np.abs(r).max()), 1e-30)
    return out


def influence(name, which, layout="perspective"):
    """Per team {tensor: distance} between the float64 reference on the real batch and on the batch with ``which`` rows' rewards negated."""
    models, _ = case_models(name)
    _, ea, _ = reference(name, layout)
    _, flipped, _ = reference(name, layout, negate=which)
    return [tensor_distances(models[t], flipped[t], ea[t], ea[t]) for t in range(2)]


def yardstick(name, layout="perspective"):
    """Per team {tensor: the float32 torch path's own distance from the float64 reference}."""
    models, _ = case_models(name)
    _, ea, _ = reference(name, layout)
    _, ea32, _ = reference(name, layout, "float32")
    return [tensor_distances(models[t], ea32[t], ea[t], ea[t]) for t in range(2)]
