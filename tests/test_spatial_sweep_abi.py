"""CPU-only checks of the SpatialDQN sweep step (susnet_spatial_train_sweep): the two symbols and their prototypes, the table query, every
host-side refusal -- each before any launch, on handles without device buffers, naming the learner and the field -- and the Python side's
argument checks (DeviceDQNSweepTrainer.compatible, sweep_chunks, run_sweep).  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

from test_spatial_train_abi import NOTEBOOK, _handle, _io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("susnet_spatial_train_sweep_table_bytes", "susnet_spatial_train_sweep")
TABLE = 1 << 24  # a plausible, 256-byte aligned, never dereferenced table address


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_sweep_symbols_are_declared_exported_and_typed(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = L.lib()
    for s in SYMBOLS:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8  # an addition: the ABI version stays
    m = re.search(r"#define SUSNET_SPATIAL_SWEEP_MAX_LEARNERS (\d+)", header)
    assert m and int(m.group(1)) == L.SPATIAL_SWEEP_MAX_LEARNERS and 8 <= L.SPATIAL_SWEEP_MAX_LEARNERS <= 16
    P = C.POINTER
    assert lib.susnet_spatial_train_sweep_table_bytes.argtypes == [C.c_int32, P(C.c_uint64)]
    assert lib.susnet_spatial_train_sweep.argtypes == [P(C.c_void_p), P(L.SpatialTrainIO), P(L.RnnDropout), C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]
    assert re.search(r"int susnet_spatial_train_sweep\(susnet_env \*const \*envs, const susnet_spatial_train_io \*ios,\s*const susnet_rnn_dropout \*drops", header)


def test_table_bytes(pkg):
    L = pkg._lib
    lib = L.lib()
    n = C.c_uint64()
    sizes = []
    for K in range(1, L.SPATIAL_SWEEP_MAX_LEARNERS + 1):
        assert lib.susnet_spatial_train_sweep_table_bytes(K, C.byref(n)) == 0, lib.susnet_last_error()
        assert n.value > 0 and n.value % 256 == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[0] < sizes[7] < sizes[-1]
    for K in (0, -1, L.SPATIAL_SWEEP_MAX_LEARNERS + 1):
        assert lib.susnet_spatial_train_sweep_table_bytes(K, C.byref(n)) == L.E_INVALID
        assert b"susnet_spatial_train_sweep_table_bytes" in lib.susnet_last_error() and b"n_learners" in lib.susnet_last_error()
    assert lib.susnet_spatial_train_sweep_table_bytes(3, None) == L.E_INVALID


def _learner(L, k, **kw):
    """A well-formed io whose written buffers are its own (distinct, aligned, never dereferenced addresses)."""
    io = _io(L, workspace=(1 << 30) + (k << 26), **kw)
    io.losses_out = (1 << 20) + 256 * k
    for t in range(2):
        if io.team[t].enabled:
            io.team[t].params = (1 << 21) + 4096 * (2 * k + t)
    return io


def _sweep(L, lib, handles, ios, drops=None, K=None, table=TABLE, table_bytes=1 << 20):
    n = len(ios)
    arr = (L.SpatialTrainIO * n)(*ios)
    envs = (C.c_void_p * n)(*handles)
    d = None
    if drops is not None:
        d = (L.RnnDropout * (2 * n))()
        for k, (p0, p1) in enumerate(drops):
            for t in range(2):
                d[2 * k + t].p[0], d[2 * k + t].p[1], d[2 * k + t].seed = p0, p1, 7 + k
    return lib.susnet_spatial_train_sweep(envs, arr, d, n if K is None else K, table, table_bytes, None)


def test_sweep_refusals_name_the_learner_and_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    hs = [h, h, h]

    def refused(ios, *words, handles=None, **kw):
        assert _sweep(L, lib, handles or hs[:len(ios)], ios, **kw) == L.E_INVALID, words
        msg = lib.susnet_last_error()
        assert msg.startswith(b"susnet_spatial_train_sweep: ") and all(w in msg for w in words), (words, msg)

    def three(edit=None, **kw):
        ios = [_learner(L, k, **kw) for k in range(3)]
        if edit is not None:
            edit(ios[2])
        return ios

    def with_(**kw):
        return dict(NOTEBOOK, **kw)

    # null arrays, K out of range
    assert lib.susnet_spatial_train_sweep(None, (L.SpatialTrainIO * 1)(), None, 1, TABLE, 1 << 20, None) == L.E_INVALID
    assert b"null envs / ios" in lib.susnet_last_error()
    assert lib.susnet_spatial_train_sweep((C.c_void_p * 1)(h), None, None, 1, TABLE, 1 << 20, None) == L.E_INVALID
    assert b"null envs / ios" in lib.susnet_last_error()
    for K in (0, L.SPATIAL_SWEEP_MAX_LEARNERS + 1):
        refused(three(), b"n_learners", K=K)
    refused(three(), b"learner 1: null handle", handles=[h, None, h])
    # what the learners must agree on, one case per field
    h4 = _handle(L, lib, n_crew=3)
    refused(three(), b"learner 2: agent count differs from learner 0's", handles=[h, h, h4])
    lib.susnet_destroy(h4)
    refused(three(lambda io: setattr(io, "n", 6)), b"learner 2: n differs from learner 0's")
    refused([_learner(L, 0), _learner(L, 1), _learner(L, 2, net1=None)], b"learner 2: team[1].enabled differs")
    for field, net in (("T", with_(T=5)), ("N", with_(N=10)), ("C", with_(C=6)), ("Fn", with_(Fn=14)), ("k", with_(k=5)),
                       ("n_conv", with_(convs=[(5, 1, 1, 1), (3, 1, 1, 1)])), ("conv_out[1]", with_(convs=[(5, 1, 1, 1), (4, 1, 1, 1), (3, 1, 1, 1)])),
                       ("conv_stride[0]", with_(convs=[(5, 2, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)])),
                       ("conv_padding[2]", with_(convs=[(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 2, 1)])),
                       ("conv_dilation[1]", with_(convs=[(5, 1, 1, 1), (3, 1, 1, 2), (3, 1, 1, 1)])), ("rnn_layers", with_(layers=2)),
                       ("rnn_hidden", with_(hidden=32, dims=[32, 16, 16, 5]))):
        refused([_learner(L, 0), _learner(L, 1), _learner(L, 2, net0=net, net1=net)], b"learner 2: net[0]." + field.encode() + b" differs from learner 0's")
    refused([_learner(L, 0), _learner(L, 1, net1=with_(dims=[64, 16, 5]))], b"learner 1: team[1].n_dims differs from learner 0's")
    refused([_learner(L, 0), _learner(L, 1, net1=with_(dims=[64, 16, 12, 5]))], b"learner 1: team[1].dims differs from learner 0's")
    refused(three(lambda io: io.spatial_stride.__setitem__(1, 0)), b"learner 2: spatial_stride[1] differs")
    refused(three(lambda io: io.non_spatial_stride.__setitem__(2, 80)), b"learner 2: non_spatial_stride[2] differs")
    refused([_learner(L, 0), _learner(L, 1)], b"learner 1: ", b"team[0] is masked", b"differs from learner 0's", drops=[(0.2, 0.0), (0.0, 0.0)])
    assert _sweep(L, lib, [h, h], [_learner(L, 0), _learner(L, 1)], drops=[(0.2, 0.0), (0.5, 0.3)], table=None) == L.E_INVALID  # (p may differ)
    assert b"table" in lib.susnet_last_error()
    # a learner that fails its own call's check: the message is carried through
    bad = with_(hidden=257, dims=[257, 16, 5])
    refused([_learner(L, 0), _learner(L, 1, net0=bad, net1=None)], b"learner 1: susnet_spatial_train_step: net[0].rnn_hidden = 257")
    refused(three(lambda io: setattr(io, "rewards", None)), b"learner 2: susnet_spatial_train_step: rewards is NULL")
    refused(three(lambda io: setattr(io, "workspace_bytes", 16)), b"learner 2: susnet_spatial_train_step: workspace")
    refused([_learner(L, 0), _learner(L, 1)], b"learner 1: susnet_spatial_train_step_dropout: drop[0].p[0]", drops=[(0.2, 0.0), (1.0, 0.0)])
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
    # the table
    refused(three(), b"table", table=None)
    refused(three(), b"table", b"256-byte aligned", table=TABLE + 128)
    n = C.c_uint64()
    assert lib.susnet_spatial_train_sweep_table_bytes(3, C.byref(n)) == 0
    refused(three(), b"table", b"smaller", table_bytes=n.value - 1)
    lib.susnet_destroy(h)


class _Env:
    """What compatible() reads of an env."""

    def __init__(self, n_agents=5, grid=None):
        self.n_agents, self.n_imposters, self.flattened_state_size = n_agents, 1, 3 * n_agents
        self.grid = torch.ones(9, 9, dtype=torch.bool) if grid is None else grid


def _cpu_trainer(pkg, desc, seed=None, spatial=True, env=None, kind="global"):
    """A DeviceDQNTeamTrainer shell with the fields compatible() reads (a real one needs a device)."""
    T = pkg.DeviceDQNTeamTrainer
    tr = T.__new__(T)
    tr.env, tr.device, tr.components, tr.trained, tr._dims = env or _Env(), torch.device("cpu"), [], [True, False], [None, None]
    tr.spatial, tr._spatial_nets, tr.rnn_dropout_seed, tr.dropout_steps, tr.targets = spatial, [desc, None], seed, 0, [None, None]
    tr._spatial_featurizer = lambda: kind
    return tr


def test_compatible_learns_the_spatial_shape_rules_and_chunks_by_the_new_constant(pkg):
    L = pkg._lib
    mk = lambda hidden=16, layers=2, p=0.0: pkg.policy.spatial_desc(pkg.SpatialDQN(9, 15, [7, 5, 3], [1, 1], [1, 1], (3, 3), [1, 1], layers, hidden, p, [16], 5))
    S = pkg.DeviceDQNSweepTrainer
    base = mk()
    assert base is not None
    assert S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk())]).compatible()
    assert not S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk(hidden=12))]).compatible()
    assert not S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk(layers=3))]).compatible()
    assert not S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk(), kind="persp")]).compatible()
    assert not S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk(), env=_Env(4))]).compatible()
    assert not S([_cpu_trainer(pkg, mk()), _cpu_trainer(pkg, mk(), spatial=False)]).compatible()
    # dropout: p and the seed may differ, whether a team is masked may not
    assert S([_cpu_trainer(pkg, mk(p=0.2), seed=1), _cpu_trainer(pkg, mk(p=0.5), seed=2)]).compatible()
    assert not S([_cpu_trainer(pkg, mk(p=0.2), seed=1), _cpu_trainer(pkg, mk(p=0.0), seed=2)]).compatible()
    # CPU members never take the sweep call
    class _Ring:
        trajectory_size, states = 2, torch.zeros(1)
    sweep = S([_cpu_trainer(pkg, mk(), spatial=False), _cpu_trainer(pkg, mk(), spatial=False)])
    for t in sweep.trainers:
        t.hip = t.dense = False
    assert sweep.compatible() and not sweep.uses_spatial([_Ring(), _Ring()]) and not sweep.uses_spatial([_Ring()])
    K = L.SPATIAL_SWEEP_MAX_LEARNERS
    chunks = pkg.trainer.sweep_chunks
    assert chunks(K, K) == [(0, K)] and chunks(K + 1, K) == [(0, K), (K, K + 1)] and chunks(3, K) == [(0, 3)]
    assert chunks(2 * K + 1, K) == [(0, K), (K, 2 * K), (2 * K, 2 * K + 1)] and chunks(3) == [(0, 3)]


class _ObsConfig:
    def __init__(self, mode, dtype=None, components=()):
        self.mode, self.dtype, self.components = mode, dtype, list(components)


class _SweepEnv:
    """What run_sweep's argument checks read of an env before anything touches a device."""
    auto_reset, rng_kind, n_agents, n_imposter_actions, n_crew_actions = True, "philox", 5, 5, 5

    def __init__(self, mode="raw"):
        self.obs_config = _ObsConfig(mode, torch.uint8 if mode == "raw" else None, ["onehot_pos"] if mode == "flat" else ())


def test_run_sweep_argument_checks(pkg, tmp_path):
    spatial = lambda env: pkg.SpatialDQN(9, 15, [7, 5, 3], [1, 1], [1, 1], (3, 3), [1, 1], 1, 16, 0.0, [16], 5)
    common = dict(num_steps=4, crew_model_factory=None, experiment_base_dir=tmp_path)
    # without featurizer_factory a SpatialDQN is refused as before, and so is a window of two states
    with pytest.raises(ValueError, match="served are reference MLPs"):
        pkg.run_sweep(lambda seed: _SweepEnv("flat"), [{"gamma": 0.9}], imposter_model_factory=spatial, components=["onehot_pos"], **common)
    with pytest.raises(ValueError, match="sequence_length=1"):
        pkg.run_sweep(lambda seed: _SweepEnv("flat"), [{"gamma": 0.9}], imposter_model_factory=spatial, components=["onehot_pos"], sequence_length=2, **common)
    # with it: the env's observation mode, an unserved model (the reason carried), the window length
    featurizer_factory = lambda env: object()
    with pytest.raises(ValueError, match="obs=ObsConfig\\('raw'"):
        pkg.run_sweep(lambda seed: _SweepEnv("flat"), [{"gamma": 0.9}], imposter_model_factory=spatial, components=[],
                      featurizer_factory=featurizer_factory, **common)
    with pytest.raises(ValueError, match="variant 0: the imposter model is not served by the spatial kernels: a SpatialDQN is served, got MLP"):
        pkg.run_sweep(lambda seed: _SweepEnv(), [{"gamma": 0.9}], imposter_model_factory=lambda env: pkg.MLP([4, 4, 5]), components=[],
                      featurizer_factory=featurizer_factory, **common)
    with pytest.raises(ValueError, match="the featurizer must be a GlobalFeaturizer / PerspectiveFeaturizer"):
        pkg.run_sweep(lambda seed: _SweepEnv(), [{"gamma": 0.9}], imposter_model_factory=spatial, components=[],
                      featurizer_factory=featurizer_factory, **common)
    with pytest.raises(ValueError, match="batch_size"):
        pkg.run_sweep(lambda seed: _SweepEnv(), [{"gamma": 0.9, "batch_size": 16}], imposter_model_factory=spatial, components=[],
                      featurizer_factory=featurizer_factory, **common)
    assert not any(tmp_path.iterdir()), "a refused sweep writes nothing"
