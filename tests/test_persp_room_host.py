"""CPU-only checks of the room-masked Perspective views (SUSNET_OBS_PERSP_ROOM / _ROOM_MASK): the host restatement
``features.room_mask_views`` against the reference-pinned fixture (tests/golden/generate_persp_room.py), its room function on grids
with unequal rooms, the two constants and the sizes ``susnet_obs_size`` reports, the refusals of every entry point but
``susnet_featurize`` -- before any launch, on a handle without device buffers --, and the Python surface.  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import persp_room_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


# ---- the restatement is the reference's -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_restatement_equals_the_reference_fixture(pkg, name):
    meta, d = U.load_fixture(name)
    A, J = meta["n_agents"], meta["n_jobs"]
    assert meta["grid_n"] == 9 and d["raw"].dtype == np.uint8 and len(d["raw"]) >= 64 + 16 and meta["played"] >= 64
    U.fixture_cases(d["raw"], A, J)
    env = U.ShapeEnv(A, J, 9)
    with_mask, non = pkg.features.room_mask_views(env, d["raw"], True)
    without, non2 = pkg.features.room_mask_views(env, d["raw"], False)
    assert with_mask.shape == (len(d["raw"]), A, A + 3, 9, 9) and without.shape == (len(d["raw"]), A, A + 2, 9, 9)
    np.testing.assert_array_equal(with_mask, d["spatial_mask"])
    np.testing.assert_array_equal(without, d["spatial"])
    np.testing.assert_array_equal(non, d["non_spatial"])
    np.testing.assert_array_equal(non2, d["non_spatial"])
    assert non.shape[-1] == (2 * A if name.startswith("tagging") else A) + J  # (tagging: two per-agent blocks)
    # the fixture's own consistency: the mask channel is the mask the other channels were multiplied by
    np.testing.assert_array_equal(d["spatial_mask"][:, :, :A + 2], d["spatial"])
    assert (d["spatial"] <= d["spatial_mask"][:, :, A + 2:]).all()


def test_restatement_takes_windows_and_torch_rows(pkg):
    meta, d = U.load_fixture("base_1v2_j4")
    env = U.ShapeEnv(meta["n_agents"], meta["n_jobs"], 9)
    rows = d["raw"][:80].reshape(20, 4, -1)
    sp, non = pkg.features.room_mask_views(env, torch.from_numpy(rows).to(torch.int64))
    np.testing.assert_array_equal(sp, d["spatial_mask"][:80].reshape(20, 4, *d["spatial_mask"].shape[1:]))
    np.testing.assert_array_equal(non, d["non_spatial"][:80].reshape(20, 4, *d["non_spatial"].shape[1:]))


@pytest.mark.parametrize("n", [14, 10, 9, 2])
def test_room_function_on_every_cell(pkg, n):
    """(x <= w, y <= w) with w = (n - 1) // 2, evaluated directly: n = 14 (w = 6: the 14 x 14 map's wall row and column are NOT the last
    row and column of the top / left rooms, the rooms are a function of n alone), n = 10 (w = 4), n = 9 (the reference's quadrants, 5 + 4
    cells a side), n = 2."""
    w = (n - 1) // 2
    rooms = pkg.features.room_index(n)
    assert rooms.shape == (n, n)
    for x in range(n):
        for y in range(n):
            assert rooms[x, y] == int(x <= w) + 2 * int(y <= w), (x, y)
    # and the restatement's masks are that function: one observer per cell, alone on the grid
    cells = np.array([(x, y) for x in range(n) for y in range(n)], dtype=np.uint8)
    raw = np.concatenate([cells, np.zeros((n * n, 2), np.uint8), np.ones((n * n, 2), np.uint8)], axis=1)  # A = 2, J = 0: x0 y0 x1 y1 alive alive
    sp, _ = pkg.features.room_mask_views(U.ShapeEnv(2, 0, n), raw, True)
    for k, (x, y) in enumerate(cells):
        want = np.array([[int((a <= w) == (x <= w) and (b <= w) == (y <= w)) for b in range(n)] for a in range(n)], dtype=np.uint8)
        np.testing.assert_array_equal(sp[k, 0, -1], want)
        assert sp[k, 0, 0, x, y] == 1 and sp[k, 0, 0].sum() == 1


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def _handle(L, lib, variant=None, n_crew=2, n_jobs=4, grid_n=9):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE if variant is None else variant, batch=8, n_imposters=1, n_crew=n_crew, n_jobs=n_jobs, grid_n=grid_n,
                     max_time_steps=1000, is_action_order_random=1, shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


def test_constants_are_declared_and_the_version_stays(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    defines = dict(re.findall(r"#define (SUSNET_[A-Z0-9_]+) (\d+)", header))
    assert int(defines["SUSNET_OBS_PERSP_ROOM"]) == L.OBS_PERSP_ROOM == 5
    assert int(defines["SUSNET_OBS_PERSP_ROOM_MASK"]) == L.OBS_PERSP_ROOM_MASK == 6
    assert int(defines["SUSNET_OBS_PERSP"]) == L.OBS_PERSP == 4
    assert int(defines["SUSNET_ABI_VERSION"]) == L.ABI_VERSION == 8


@pytest.mark.parametrize("game", [("base", 2, 4, 14), ("tagging", 4, 5, 9), ("base", 11, 3, 9)])
def test_obs_size(pkg, game):
    L = pkg._lib
    lib = L.lib()
    kind, n_crew, J, N = game
    A = 1 + n_crew
    h = _handle(L, lib, L.VARIANT_TAGGING if kind == "tagging" else None, n_crew, J, N)
    sizes = {}
    for mode in (L.OBS_PERSP, L.OBS_PERSP_ROOM, L.OBS_PERSP_ROOM_MASK):
        spec = L.ObsSpec()
        spec.mode, spec.dtype = mode, L.U8
        f1, f2 = C.c_int32(0), C.c_int32(0)
        assert lib.susnet_obs_size(h, C.byref(spec), C.byref(f1), C.byref(f2)) == 0, lib.susnet_last_error()
        sizes[mode] = (f1.value, f2.value)
    assert sizes[L.OBS_PERSP_ROOM] == (A * (A + 2) * N * N, sizes[L.OBS_PERSP][1]) == sizes[L.OBS_PERSP]
    assert sizes[L.OBS_PERSP_ROOM_MASK] == (A * (A + 3) * N * N, sizes[L.OBS_PERSP][1])
    assert sizes[L.OBS_PERSP][1] == A * ((2 * A if kind == "tagging" else A) + J)
    lib.susnet_destroy(h)


@pytest.mark.parametrize("mode_name", ["SUSNET_OBS_PERSP_ROOM", "SUSNET_OBS_PERSP_ROOM_MASK"])
def test_every_entry_point_but_featurize_refuses_the_modes_before_any_launch(pkg, mode_name):
    """On a handle without a state blob (nothing could be launched: every one of these calls needs the bound state, and says so for any
    other observation mode): SUSNET_E_INVALID, naming the mode, ahead of the state check."""
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    buf = (C.c_uint8 * 64)()
    spec = L.ObsSpec()
    spec.mode, spec.dtype = getattr(L, mode_name[len("SUSNET_"):]), L.U8
    spec.out = (C.addressof(buf) + 15) & ~15
    step_io, roll_io = L.StepIO(), L.RolloutIO()
    step_io.actions, step_io.obs = spec.out, C.pointer(spec)
    roll_io.n_ticks, roll_io.obs = 2, C.pointer(spec)
    calls = {"susnet_reset": lambda: lib.susnet_reset(h, None, C.byref(spec), None),
             "susnet_step": lambda: lib.susnet_step(h, C.byref(step_io), None),
             "susnet_policy_step": lambda: lib.susnet_policy_step(h, spec.out, None, None, C.byref(step_io), None),
             "susnet_rollout": lambda: lib.susnet_rollout(h, C.byref(roll_io), None),
             "susnet_observe": lambda: lib.susnet_observe(h, C.byref(spec), None)}
    for name, call in calls.items():
        assert call() == L.E_INVALID, name
        msg = lib.susnet_last_error().decode()
        assert mode_name + " " in msg and "susnet_featurize" in msg, (name, msg)
        assert name.replace("susnet_policy_step", "policy tick") in msg, (name, msg)
    # the same calls with the plain Perspective mode get as far as the state check
    spec.mode = L.OBS_PERSP
    for name, call in calls.items():
        assert call() == L.E_STATE, name
    lib.susnet_destroy(h)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def test_obs_config_accepts_the_modes(pkg):
    L = pkg._lib
    assert pkg.ObsConfig("persp_room").code == L.OBS_PERSP_ROOM and pkg.ObsConfig("persp_room_mask", dtype=torch.uint8).code == L.OBS_PERSP_ROOM_MASK
    assert pkg.ObsConfig("persp").code == L.OBS_PERSP
    with pytest.raises(AssertionError):
        pkg.ObsConfig("persp_rooms")


class _NoDevice:
    """``_make_obs`` on a library handle alone (its tensors on the CPU): the shapes it gives the modes."""

    def __init__(self, pkg, n_crew, n_jobs, n, variant=None):
        L = pkg._lib
        self.lib, self.batch, self.n_agents, self.n_rows, self.device = L.lib(), 8, 1 + n_crew, n, torch.device("cpu")
        self._h = _handle(L, self.lib, variant, n_crew, n_jobs, n)


def test_make_obs_shapes(pkg):
    L = pkg._lib
    for n_crew, J, N, variant in ((2, 4, 14, None), (4, 5, 9, L.VARIANT_TAGGING)):
        env = _NoDevice(pkg, n_crew, J, N, variant)
        A = 1 + n_crew
        F2 = (2 * A if variant is not None else A) + J
        make = lambda mode, **kw: pkg.BatchedFourRoomEnv._make_obs(env, pkg.ObsConfig(mode, dtype=torch.uint8), 1, **kw)
        _, o1, o2 = make("persp_room", rows=5)
        assert tuple(o1.shape) == (5, A, A + 2, N, N) and tuple(o2.shape) == (5, A, F2) and o1.dtype == torch.uint8
        _, o1, o2 = make("persp_room_mask", rows=5)
        assert tuple(o1.shape) == (5, A, A + 3, N, N) and tuple(o2.shape) == (5, A, F2)
        _, o1, o2 = make("persp_room_mask")
        assert tuple(o1.shape) == (8, A, A + 3, N, N) and tuple(o2.shape) == (8, A, F2)
        _, o1, o2 = make("persp", rows=5)  # as it was
        assert tuple(o1.shape) == (5, A, A + 2, N, N) and tuple(o2.shape) == (5, A, F2)
        env.lib.susnet_destroy(env._h)


@pytest.mark.parametrize("mode", ["persp_room", "persp_room_mask"])
def test_an_env_built_with_the_modes_is_refused(pkg, mode):
    with pytest.raises(ValueError, match="featurize raw rows"):
        pkg.BatchedFourRoomEnv(1, 2, 4, batch=8, obs=pkg.ObsConfig(mode))


def test_the_default_perspective_featurizer_is_what_it_was(pkg):
    env = U.ShapeEnv(3, 4, 9)
    f = pkg.PerspectiveFeaturizer(env)
    assert f.config.mode == "persp" and f.config.dtype == torch.float32 and f.config.components == [] and not f.partially_observable
    assert pkg.PerspectiveFeaturizer(env, partially_observable=True).config.mode == "persp_room_mask"
    assert pkg.PerspectiveFeaturizer(env, True, add_obs_mask_feature=False).config.mode == "persp_room"
    assert pkg.PerspectiveFeaturizer(env, False, add_obs_mask_feature=False).config.mode == "persp"
    assert callable(pkg.features.room_mask_views)


def test_the_acting_test_seeds_have_few_near_ties_on_the_torch_module_alone(pkg):
    """tests/test_gpu_persp_room.py compares actions where no two Q values lie within the kernel tolerance (2e-5 of the largest |Q|) and
    asserts that at most 5 % of rows are so excluded: its models (persp_room_util.acting_models, ACTING_SEEDS) satisfy that by themselves,
    on windows of the fixture's tagging 1v4 rows, with room to spare (here: at most 1 %)."""
    L = pkg._lib
    meta, d = U.load_fixture("tagging_1v4_j5")
    A, J = meta["n_agents"], meta["n_jobs"]
    h = _handle(L, L.lib(), L.VARIANT_TAGGING, 4, 5, 9)
    lay = L.Layout()
    assert L.lib().susnet_get_layout(h, C.byref(lay)) == 0
    models = U.acting_models(pkg, A, 9, 2 * A + J, lay.n_actions_imposter, lay.n_actions_crew, "cpu")
    L.lib().susnet_destroy(h)
    windows = np.stack([d["raw"][:-1], d["raw"][1:]], axis=1)  # [81, T = 2, S]
    sp, non = pkg.features.room_mask_views(U.ShapeEnv(A, J, 9), windows, True)
    sp, non = torch.from_numpy(sp).float(), torch.from_numpy(non).float()
    for m in models:
        with torch.no_grad():
            q = torch.cat([m(sp[:, :, i], non[:, :, i]) for i in range(A)])
        top = q.topk(2, dim=1).values
        near = (top[:, 0] - top[:, 1]) <= 2e-5 * float(q.abs().max())
        assert float(near.float().mean()) <= 0.01, float(near.float().mean())
