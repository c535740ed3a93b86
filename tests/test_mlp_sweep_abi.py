"""CPU-only checks of the dense learner's sweep step (susnet_mlp_train_sweep): the symbol and its prototype, every host-side refusal --
each before any launch, on handles without device buffers, naming the learner and the field -- and the Python side's argument checks and
host logic (run_sweep, DeviceDQNSweepTrainer's dispatch order and chunks).  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

from test_mlp_train_abi import _handle, _io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_sweep_symbol_is_declared_exported_and_typed(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = L.lib()
    assert "susnet_mlp_train_sweep" in declared and "susnet_mlp_train_sweep" in L.EXPORTS and hasattr(lib, "susnet_mlp_train_sweep")
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8  # an addition: the ABI version stays
    m = re.search(r"#define SUSNET_MLP_SWEEP_MAX_LEARNERS (\d+)", header)
    assert m and int(m.group(1)) == L.MLP_SWEEP_MAX_LEARNERS == 16
    P = C.POINTER
    assert lib.susnet_mlp_train_sweep.argtypes == [P(C.c_void_p), P(L.MlpTrainIO), C.c_int32, C.c_void_p]
    assert re.search(r"int susnet_mlp_train_sweep\(susnet_env \*const \*envs, const susnet_mlp_train_io \*ios, int32_t n_learners, void \*stream\);", header)


def _learner(L, k, **kw):
    """A well-formed io whose written buffers are its own (distinct, aligned, never dereferenced addresses)."""
    io = _io(L, workspace=(1 << 30) + (k << 26), **kw)
    io.losses_out = (1 << 20) + 256 * k
    for t in range(2):
        if io.team[t].enabled:
            io.team[t].params = (1 << 21) + 4096 * (2 * k + t)
    return io


def _sweep(L, lib, handles, ios, K=None):
    n = len(ios)
    arr = (L.MlpTrainIO * n)(*ios)
    envs = (C.c_void_p * n)(*handles)
    return lib.susnet_mlp_train_sweep(envs, arr, n if K is None else K, None)


def test_sweep_refusals_name_the_learner_and_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    hs = [h, h, h]

    def refused(ios, *words, handles=None, **kw):
        assert _sweep(L, lib, handles or hs[:len(ios)], ios, **kw) == L.E_INVALID, words
        msg = lib.susnet_last_error()
        assert msg.startswith(b"susnet_mlp_train_sweep: ") and all(w in msg for w in words), (words, msg)

    def three(edit=None, **kw):
        ios = [_learner(L, k, **kw) for k in range(3)]
        if edit is not None:
            edit(ios[2])
        return ios

    # null arrays (a null io array among them), K out of range, a null handle
    assert lib.susnet_mlp_train_sweep(None, (L.MlpTrainIO * 1)(), 1, None) == L.E_INVALID
    assert b"susnet_mlp_train_sweep: null envs / ios" in lib.susnet_last_error()
    assert lib.susnet_mlp_train_sweep((C.c_void_p * 1)(h), None, 1, None) == L.E_INVALID
    assert b"susnet_mlp_train_sweep: null envs / ios" in lib.susnet_last_error()
    for K in (0, -1, L.MLP_SWEEP_MAX_LEARNERS + 1):
        refused(three(), b"n_learners", b"outside 1 .. 16", K=K)
    refused(three(), b"learner 1: null handle", handles=[h, None, h])
    # what the learners must agree on, one case per field
    other = [36, 256, 128, 64, 32, 6]
    refused([_learner(L, 0), _learner(L, 1, dims0=other)], b"learner 1: team[0].dims differs from learner 0's")
    refused([_learner(L, 0), _learner(L, 1, dims1=[36, 64, 6])], b"learner 1: team[1].n_dims differs from learner 0's")
    refused(three(lambda io: setattr(io, "n", 6)), b"learner 2: n differs from learner 0's")
    refused([_learner(L, 0), _learner(L, 1), _learner(L, 2, dims1=None)], b"learner 2: team[1].enabled differs from learner 0's")
    refused([_learner(L, 0, dims0=None), _learner(L, 1)], b"learner 1: team[0].enabled differs from learner 0's")
    h5 = _handle(L, lib, n_crew=4)
    refused(three(), b"learner 2: agent count differs from learner 0's", handles=[h, h, h5])
    lib.susnet_destroy(h5)
    # no two learners write the same memory
    ios = three()
    ios[2].team[0].params = ios[1].team[1].params
    refused(ios, b"learner 2: team[0].params is shared with learner 1")
    ios = three()
    ios[1].workspace = ios[0].workspace
    refused(ios, b"learner 1: workspace is shared with learner 0")
    ios = three()
    ios[2].losses_out = ios[0].losses_out
    refused(ios, b"learner 2: losses_out is shared with learner 0")
    # a learner that the single call refuses: its message is carried through
    ios = [_learner(L, 0), _learner(L, 1)]
    ios[1].team[1].packed = 4096
    refused(ios, b"learner 1: susnet_mlp_train_step: team[1].packed must be NULL")
    refused(three(lambda io: setattr(io, "rewards", None)), b"learner 2: susnet_mlp_train_step: rewards is NULL")
    refused(three(lambda io: setattr(io, "workspace_bytes", 16)), b"learner 2: susnet_mlp_train_step: workspace")
    refused([_learner(L, 0), _learner(L, 1, dims0=[36, 257, 6], dims1=None)], b"learner 1: susnet_mlp_train_step: team[0].dims[1]", b"hidden")
    h2 = _handle(L, lib, n_imposters=2, n_crew=3)
    refused(three(), b"learner 1: susnet_mlp_train_step: n_imposters", handles=[h, h2, h])
    lib.susnet_destroy(h2)
    lib.susnet_destroy(h)


class _ObsConfig:
    mode, components = "flat", ["onehot_pos"]


class _SweepEnv:
    """What run_sweep reads of an env before anything touches a device."""
    auto_reset, rng_kind, obs_config = True, "philox", _ObsConfig()


class _Reached(Exception):
    pass


def test_run_sweep_lets_a_dense_sweep_read_windows(pkg, tmp_path):
    def model_factory(env):
        raise _Reached()

    common = dict(num_steps=4, crew_model_factory=None, experiment_base_dir=tmp_path, imposter_model_factory=model_factory, components=["onehot_pos"])
    seeds = []
    env_factory = lambda seed: seeds.append(seed) or _SweepEnv()
    # dense_train=True: a window of two states no longer stops at the sequence_length=1 refusal -- the factories are reached
    with pytest.raises(_Reached):
        pkg.run_sweep(env_factory, [{"gamma": 0.9, "seed": 5}], sequence_length=2, dense_train=True, **common)
    assert seeds == [5]
    # dense_train=False: refused as before, before any factory is called
    with pytest.raises(ValueError, match="sequence_length=1"):
        pkg.run_sweep(env_factory, [{"gamma": 0.9, "seed": 6}], sequence_length=2, **common)
    assert seeds == [5]
    with pytest.raises(ValueError, match="served are reference MLPs"):
        pkg.run_sweep(env_factory, [{"gamma": 0.9}], sequence_length=2, dense_train=True,
                      **dict(common, imposter_model_factory=lambda env: torch.nn.Linear(2, 2)))
    assert not any(tmp_path.iterdir()), "a refused sweep writes nothing"


class _Ring:
    trajectory_size, states = 1, torch.zeros(1)


def _stub_sweep(pkg, K, hip=False, spatial=False, dense=False, compatible=True):
    """A DeviceDQNSweepTrainer over K member stubs whose paths are switched by hand; every call is written into `log`."""
    log = []

    class _Member:
        def __init__(self, k):
            self.k = k

        uses_hip = lambda self, ring: hip
        uses_spatial = lambda self, ring: spatial
        uses_dense = lambda self, ring: dense

        def train_step_on_indices(self, ring, idx):
            log.append(("own", self.k))
            return torch.zeros(2)

    sweep = pkg.DeviceDQNSweepTrainer([_Member(k) for k in range(K)])
    sweep.compatible = lambda: compatible
    sweep._spatial_sweep_step = lambda rings, idxs: log.append("spatial") or torch.zeros(K, 2)
    sweep._dense_sweep_step = lambda rings, idxs: log.append("dense") or torch.zeros(K, 2)
    return sweep, log


def test_dispatch_order_and_chunks(pkg):
    L = pkg._lib
    rings, idxs = [_Ring(), _Ring()], [torch.zeros(3, dtype=torch.int64)] * 2
    # spatial before dense; dense before the loop; nothing of the kind: the loop
    for kw, want in ((dict(spatial=True, dense=True), ["spatial"]), (dict(dense=True), ["dense"]), (dict(), [("own", 0), ("own", 1)]),
                     (dict(dense=True, compatible=False), [("own", 0), ("own", 1)])):
        sweep, log = _stub_sweep(pkg, 2, **kw)
        sweep.train_step_on_indices(rings, idxs)
        assert log == want, (kw, log)
    # the fused sweep goes first: neither of the other two is asked
    sweep, log = _stub_sweep(pkg, 2, hip=True, spatial=True, dense=True)
    assert sweep.uses_hip(rings) and not log
    # unequal index counts, or windows of two lengths: the loop
    sweep, log = _stub_sweep(pkg, 2, dense=True)
    sweep.train_step_on_indices(rings, [torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)])
    assert log == [("own", 0), ("own", 1)]
    long = _Ring()
    long.trajectory_size = 2
    assert sweep.uses_dense(rings) and not sweep.uses_dense([_Ring(), long]) and not sweep.uses_dense(rings[:1])
    # _dense_sweep_step: chunks of at most MLP_SWEEP_MAX_LEARNERS, every member prepared once, in order, and finished behind the calls
    K = 2 * L.MLP_SWEEP_MAX_LEARNERS + 3
    calls = []

    class _Env:
        _h, lib = None, None

        @staticmethod
        def _stream():
            return None

    class _Lib:
        @staticmethod
        def susnet_mlp_train_sweep(envs, ios, n, stream):
            calls.append(("call", n, len(ios)))
            return 0

    _Env.lib = _Lib

    class _Trainer:
        env, device = _Env, torch.device("cpu")

        def __init__(self, k):
            self.k = k

        def _dense_prepare(self, ring, idx):
            calls.append(("prepare", self.k))
            return L.MlpTrainIO()

        def _dense_finish(self):
            calls.append(("finish", self.k))

    sweep = pkg.DeviceDQNSweepTrainer([_Trainer(k) for k in range(K)])
    import contextlib
    real = torch.cuda.device
    torch.cuda.device = lambda d: contextlib.nullcontext()
    try:
        out = sweep._dense_sweep_step([_Ring()] * K, [torch.zeros(3, dtype=torch.int64)] * K)
    finally:
        torch.cuda.device = real
    assert out.shape == (K, 2)
    M = L.MLP_SWEEP_MAX_LEARNERS
    want = []
    for lo, hi in ((0, M), (M, 2 * M), (2 * M, K)):
        want += [("prepare", k) for k in range(lo, hi)] + [("call", hi - lo, hi - lo)]
    assert calls == want + [("finish", k) for k in range(K)]
    assert pkg.trainer.sweep_chunks(K, M) == [(0, M), (M, 2 * M), (2 * M, K)]
