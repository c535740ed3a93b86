"""CPU-only checks of ACTING under dropout between the SpatialDQN's RNN layers: the two new symbols (declared, exported, prototyped), the
unchanged ABI version and struct sizes, every host-side refusal of susnet_spatial_forward_dropout and susnet_spatial_act_dropout_mask
(before any launch, on a handle without device buffers, naming the field), how a seeded SpatialQNet resolves p from its module's mode, and
run_experiment's argument checks.  No kernel is launched here."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import pytest
import torch

from spatial_act_dropout_util import make_act_drop
from test_spatial_abi import _handle, _io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("susnet_spatial_forward_dropout", "susnet_spatial_act_dropout_mask")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


class _NoDevice:  # what SpatialQNet reads of an env before anything is launched
    device = torch.device("cpu")


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = L.lib()
    for s in SYMBOLS:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    P = C.POINTER
    assert lib.susnet_spatial_forward_dropout.argtypes == [C.c_void_p, P(L.SpatialIO), P(L.RnnDropout), C.c_int32, C.c_void_p]
    assert lib.susnet_spatial_act_dropout_mask.argtypes == [C.c_void_p, P(L.RnnDropout), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                                            C.c_int32, C.c_void_p, C.c_void_p]
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8 == L.ABI_VERSION
    # the header no longer says that acting has no dropout form, and states the acting coordinates
    assert "no dropout form of it exists" not in header
    for word in ("r % A", "row_base + r / A", "net    = 2 for the imposters", "susnet_spatial_forward_dropout"):
        assert word in header, word


def test_the_structs_kept_their_sizes(pkg, tmp_path):
    L = pkg._lib
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include "susnet.h"\nint main(void){printf("%zu %zu %d\\n", sizeof(susnet_spatial_io), '
                    'sizeof(susnet_rnn_dropout), SUSNET_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    io_size, drop_size, abi = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert io_size == C.sizeof(L.SpatialIO) == 592 and drop_size == C.sizeof(L.RnnDropout) == 32 and abi == 8


# ---- 2. the refusals -------------------------------------------------------------------------------------------------------------------------
def test_forward_dropout_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    entry = b"susnet_spatial_forward_dropout"

    def refused(drop, net, *fields, **over):
        rc = lib.susnet_spatial_forward_dropout(h, C.byref(_io(L, **over)), None if drop is None else C.byref(drop), net, None)
        msg = lib.susnet_last_error()
        assert rc == L.E_INVALID and msg.startswith(entry + b": ") and all(f in msg for f in fields), (rc, fields, msg)
        return msg

    good = lambda net=2, **kw: make_act_drop(L, kw.pop("p", 0.2), net, **kw)
    refused(None, 2, b"drop is NULL")
    for net in (-1, 0, 1, 4):
        refused(good(), net, f"net = {net}".encode())
    for net in (2, 3):  # p = drop->p[net - 2]; the other p (7.0 in make_act_drop) is not looked at
        for p in (1.0, -0.1, float("nan"), 1.5):
            refused(good(net, p=p), net, f"drop->p[{net - 2}]".encode())
    refused(good(offset=1 << 56), 2, b"drop->offset")
    refused(good(row_base=-1), 2, b"drop->row_base")
    refused(good(row_base=(1 << 40) - 7), 2, b"drop->row_base")  # n = 40 rows of 5 agents: 8 envs
    refused(good(3, row_base=1 << 40), 3, b"drop->row_base")
    refused(good(), 2, b"agents = 4097", agents=4097, n=4097)
    # the LDS rule of this form, the bytes in the message: (L + 3) buffers from three layers on, (L + 2) at two
    msg = refused(good(), 2, b"LDS under dropout", b"rnn_layers + 3", str(6 * 64 * 128 * 4).encode(), rnn_hidden=128, dims=(0, 128))
    assert b"163840" in msg
    refused(good(3), 3, b"LDS under dropout", b"rnn_layers + 2", str(4 * 64 * 256 * 4).encode(), rnn_hidden=256, dims=(0, 256), rnn_layers=2)
    # ... and the plain call's rule where the plain kernels would run: p = 0, a positive p below 2^-32
    for p in (0.0, 2.0 ** -40):
        msg = refused(good(p=p), 2, b"LDS: (rnn_layers + 1)", str(3 * 64 * 256 * 4).encode(), rnn_hidden=256, dims=(0, 256), rnn_layers=2)
        assert b"under dropout" not in msg
    # everything susnet_spatial_forward refuses, with its own message behind this call's name
    plain = b"susnet_spatial_forward"
    cases = [dict(T=9), dict(N=17), dict(k=4), dict(conv_out=(1, 33)), dict(Fn=-1), dict(rnn_layers=5), dict(rnn_hidden=257, dims=(0, 257)),
             dict(n_dims=9), dict(dims=(3, 33)), dict(n=0), dict(agents=0), dict(spatial_stride=(1, -1)), dict(w_hh=(1, None)), dict(weight=(0, 4098)),
             dict(slope=(1, None)), dict(spatial=None), dict(non_spatial=4097), dict(rnn_in=None), dict(q_out=4097),
             dict(C=32, N=16, k=1, conv_padding=[(0, 8), (1, 8)], conv_out=[(0, 32), (1, 32)], conv_stride=(2, 4))]
    for over in cases:
        assert lib.susnet_spatial_forward(h, C.byref(_io(L, **over)), None) == L.E_INVALID
        want = lib.susnet_last_error()
        assert want.startswith(plain + b": ")
        for net in (2, 3):
            assert refused(good(net), net, **over) == entry + want[len(plain):], over
    assert lib.susnet_spatial_forward_dropout(None, C.byref(_io(L)), C.byref(good()), 2, None) == L.E_INVALID
    assert lib.susnet_spatial_forward_dropout(h, None, C.byref(good()), 2, None) == L.E_INVALID
    lib.susnet_destroy(h)


def test_act_mask_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    entry = b"susnet_spatial_act_dropout_mask"
    ok = dict(net=2, agents=3, layers=3, n=7, T=3, H=33)

    def refused(drop, *fields, out=4096, **kw):
        a = dict(ok, **kw)
        rc = lib.susnet_spatial_act_dropout_mask(h, None if drop is None else C.byref(drop), a["net"], a["agents"], a["layers"], a["n"], a["T"], a["H"],
                                                 out, None)
        msg = lib.susnet_last_error()
        assert rc == L.E_INVALID and entry in msg and all(f in msg for f in fields), (rc, fields, msg)

    good = make_act_drop(L, 0.2, 2)
    refused(None, b"drop is NULL")
    for kw, field in ((dict(net=0), b"net = 0"), (dict(net=1), b"net = 1"), (dict(net=4), b"net = 4"), (dict(agents=0), b"agents = 0"),
                      (dict(agents=4097), b"agents = 4097"), (dict(layers=1), b"layers = 1"), (dict(layers=5), b"layers = 5"), (dict(n=0), b"n = 0"),
                      (dict(T=0), b"T = 0"), (dict(T=9), b"T = 9"), (dict(H=0), b"H = 0"), (dict(H=257), b"H = 257")):
        refused(good, field, **kw)
    for p in (1.0, -0.5, float("nan")):
        refused(make_act_drop(L, p, 3), b"drop->p[1]", net=3)
    refused(make_act_drop(L, 0.2, 2, offset=1 << 56), b"drop->offset")
    refused(make_act_drop(L, 0.2, 2, row_base=-1), b"drop->row_base")
    refused(make_act_drop(L, 0.2, 2, row_base=(1 << 40) - 2), b"drop->row_base")  # 7 rows of 3 agents: 3 envs
    refused(good, b"out", out=None)
    refused(good, b"out", b"4-byte", out=4098)
    assert lib.susnet_spatial_act_dropout_mask(None, C.byref(good), 2, 3, 3, 7, 3, 33, 4096, None) == L.E_INVALID
    # the train step's export keeps refusing the acting nets
    assert lib.susnet_rnn_dropout_mask(h, C.byref(good), 2, 0, 3, 7, 3, 33, 4096, None) == L.E_INVALID and b"net = 2" in lib.susnet_last_error()
    lib.susnet_destroy(h)


# ---- 3. Python ---------------------------------------------------------------------------------------------------------------------------------
def _model(pkg, layers, dropout):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return pkg.SpatialDQN(9, 15, [7, 5, 3], [1, 1], [1, 1], (3, 3), [1, 1], layers, 64, dropout, [16, 16], 5)


def test_spatial_qnet_resolves_p_by_the_modules_mode(pkg):
    Q = pkg.policy.SpatialQNet
    assert inspect.signature(Q.__new__).parameters["act_dropout_seed"].default is None
    fwd = inspect.signature(Q.forward).parameters
    assert (fwd["net"].default, fwd["offset"].default, fwd["row_base"].default) == (2, 0, 0)
    # without a seed: as before -- no dropout, and a training-mode model with dropout between several layers raises
    m = _model(pkg, 3, 0.2)
    net = Q(_NoDevice(), m)
    assert net.act_dropout_seed is None and net.act_dropout_p() == 0.0
    with pytest.raises(RuntimeError, match="training mode"):
        net.forward(torch.zeros(1, 2, 7, 9, 9), torch.zeros(1, 2, 15))
    # with a seed the call follows the module's mode, as torch does
    net = Q(_NoDevice(), m, act_dropout_seed=5)
    assert m.training and net.act_dropout_seed == 5 and net.act_dropout_p() == pytest.approx(0.2)
    m.eval()
    assert net.act_dropout_p() == 0.0
    m.train()
    assert net.act_dropout_p() == pytest.approx(0.2)
    assert Q(_NoDevice(), _model(pkg, 1, 0.2), act_dropout_seed=5).act_dropout_p() == 0.0  # one layer: nothing to drop
    assert Q(_NoDevice(), _model(pkg, 3, 0.0), act_dropout_seed=5).act_dropout_p() == 0.0  # rnn_dropout = 0
    assert Q(_NoDevice(), m, act_dropout_seed=-1).act_dropout_seed == 2 ** 64 - 1  # (the key is 64 bits)


def test_the_python_arguments(pkg, tmp_path):
    tl = pkg.train_loop
    for fn in (pkg.WindowedPolicyRollout.__init__, tl.run_experiment):
        assert inspect.signature(fn).parameters["act_dropout_seed"].default is None, fn
    for fn in (tl.run_sweep, tl.evaluate, tl.evaluate_checkpoints):  # out of scope, and said so
        assert "act_dropout_seed" not in inspect.signature(fn).parameters
    assert "act_dropout_seed" in tl.run_experiment.__doc__ and "act_dropout_seed" in tl.evaluate.__doc__
    assert "act_ticks" in pkg.DeviceReplayBuffer.collect.__doc__
    assert [f.name for f in __import__("dataclasses").fields(tl._Settings)][-3:] == ["rnn_dropout_seed", "act_dropout_seed", "seed"]
    # without a featurizer there is nothing to seed: refused before anything is built or written
    with pytest.raises(ValueError, match="act_dropout_seed"):
        tl.run_experiment(None, 10, None, None, ["onehot_pos"], experiment_base_dir=tmp_path, act_dropout_seed=3)
    assert list(tmp_path.iterdir()) == []
