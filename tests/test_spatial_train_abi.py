"""CPU-only checks of the SpatialDQN train step (susnet_spatial_train_step): the structs against their ctypes mirrors, the two symbols, the
workspace query on both fixture networks, and the host-side refusals -- every one before any launch, on a handle without device buffers,
naming the field.  No kernel is launched here."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("susnet_spatial_train_workspace_bytes", "susnet_spatial_train_step")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_spatial_train_io_matches_the_header(pkg, tmp_path):
    L = pkg._lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(susnet_spatial_train_io));', 'printf("net_size %zu\\n", sizeof(susnet_spatial_net));',
             'printf("team_size %zu\\n", sizeof(susnet_dqn_team));', 'printf("abi %d\\n", SUSNET_ABI_VERSION);',
             'printf("max_grid %d\\n", SUSNET_SPATIAL_TRAIN_MAX_GRID);']
    for fname, _ in L.SpatialTrainIO._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_spatial_train_io, {fname}));')
    for fname, _ in L.SpatialNet._fields_:
        lines.append(f'printf("net.{fname} %zu\\n", offsetof(susnet_spatial_net, {fname}));')
    lines += ["return 0;}"]
    prog = tmp_path / "spatial_train_io.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "spatial_train_io"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.SpatialTrainIO)
    assert int(out["net_size"]) == C.sizeof(L.SpatialNet)
    assert int(out["team_size"]) == C.sizeof(L.DqnTeam)
    for fname, _ in L.SpatialTrainIO._fields_:
        assert int(out[fname]) == getattr(L.SpatialTrainIO, fname).offset, fname
    for fname, _ in L.SpatialNet._fields_:
        assert int(out["net." + fname]) == getattr(L.SpatialNet, fname).offset, fname
    assert int(out["abi"]) == 8 == L.ABI_VERSION  # additions only: the ABI version stays
    assert int(out["max_grid"]) == L.SPATIAL_TRAIN_MAX_GRID


def test_spatial_train_symbols_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in pkg._lib.EXPORTS and hasattr(lib, s), s
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8


def _handle(L, lib, n_imposters=1, n_crew=4):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=8, n_imposters=n_imposters, n_crew=n_crew, n_jobs=4, grid_n=9, max_time_steps=1000,
                     is_action_order_random=1, shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


# the two networks of tests/golden/generate_spatial.py: the notebook's (Global featurizer, 9x9, T = 6, channels [7, 5, 3] with the repeated
# last layer, k = 3, three RNN layers of 64, head [64, 16, 16, n]) and the Perspective one (14x14, T = 3, [5, 6, 8], one layer of 16, [16, 12, n])
NOTEBOOK = dict(T=6, N=9, C=7, Fn=15, k=3, convs=[(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], layers=3, hidden=64, dims=[64, 16, 16, 5])
PERSPECTIVE = dict(T=3, N=14, C=5, Fn=6, k=3, convs=[(6, 1, 1, 1), (8, 1, 1, 1), (8, 1, 1, 1)], layers=1, hidden=16, dims=[16, 12, 5])


def _io(L, net0=NOTEBOOK, net1=NOTEBOOK, n=5, ptr=4096, workspace=1 << 20):
    """A well-formed susnet_spatial_train_io whose pointers are plausible, aligned, never dereferenced values (every step call below is refused)."""
    io = L.SpatialTrainIO()
    for name in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        setattr(io, name, ptr)
    io.max_size, io.n, io.gamma = 64, n, 0.9
    for t, d in enumerate((net0, net1)):
        if d is None:
            continue
        tm, net = io.team[t], io.net[t]
        tm.enabled, tm.n_dims = 1, len(d["dims"])
        for k, v in enumerate(d["dims"][:8]):
            tm.dims[k] = v
        tm.lr, tm.beta1, tm.beta2, tm.eps = 1e-3, 0.9, 0.999, 1e-8
        tm.params = tm.target_params = tm.exp_avg = tm.exp_avg_sq = tm.step = ptr
        net.T, net.N, net.C, net.Fn, net.k, net.n_conv = d["T"], d["N"], d["C"], d["Fn"], d["k"], len(d["convs"])
        for l, (co, st, pad, dil) in enumerate(d["convs"][:4]):
            net.conv_out[l], net.conv_stride[l], net.conv_padding[l], net.conv_dilation[l] = co, st, pad, dil
        net.rnn_layers, net.rnn_hidden = d["layers"], d["hidden"]
    A = 5
    img = net0["C"] * net0["N"] ** 2
    for k, v in enumerate((net0["T"] * A * img, img, A * img)):
        io.spatial_stride[k] = v
    for k, v in enumerate((net0["T"] * A * net0["Fn"], net0["Fn"], A * net0["Fn"])):
        io.non_spatial_stride[k] = v
    io.workspace, io.workspace_bytes = workspace, 1 << 40
    return io


def test_workspace_query_serves_both_fixture_networks_without_a_device(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    nbytes = C.c_uint64()
    sizes = {}
    for name, d in (("notebook", NOTEBOOK), ("perspective", PERSPECTIVE)):
        for n in (0, 32, 4096):
            assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(_io(L, d, d, n=n)), C.byref(nbytes)) == 0, (name, lib.susnet_last_error())
            assert nbytes.value > 0 and nbytes.value % 256 == 0
            sizes[name, n] = nbytes.value
        assert sizes[name, 0] < sizes[name, 32] < sizes[name, 4096]
    # the widest served network at the largest batch: the byte count does not overflow
    wide = dict(T=8, N=16, C=32, Fn=0, k=5, convs=[(32, 1, 2, 1)] * 3 + [(16, 1, 2, 1)], layers=4, hidden=256, dims=[256] * 7 + [32])
    assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(_io(L, wide, wide, n=1 << 30)), C.byref(nbytes)) == 0, lib.susnet_last_error()
    assert nbytes.value > (1 << 30) * 8 * 4096 * 4
    lib.susnet_destroy(h)


def test_spatial_train_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound: the call needs none)
    nbytes = C.c_uint64()

    def refused(io, *fields, handle=h):
        assert lib.susnet_spatial_train_step(handle, C.byref(io), None) == L.E_INVALID, fields
        msg = lib.susnet_last_error()
        assert b"susnet_spatial_train_step" in msg and all(f in msg for f in fields), (fields, msg)

    def plan_refused(io, *fields, handle=h):
        """Refused by the workspace query too: the networks, n and the handle are checked there."""
        assert lib.susnet_spatial_train_workspace_bytes(handle, C.byref(io), C.byref(nbytes)) == L.E_INVALID, fields
        assert all(f in lib.susnet_last_error() for f in fields), (fields, lib.susnet_last_error())
        refused(io, *fields, handle=handle)

    def with_(base, **kw):
        return dict(base, **kw)

    assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(_io(L)), C.byref(nbytes)) == 0, lib.susnet_last_error()
    plan_refused(_io(L, with_(NOTEBOOK, T=9), None), b"net[0].T = 9")
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, k=2)), b"net[1].k = 2")
    plan_refused(_io(L, with_(NOTEBOOK, N=17), None), b"net[0].N = 17")
    plan_refused(_io(L, with_(NOTEBOOK, C=33), None), b"net[0].C = 33")
    io = _io(L)
    io.net[0].n_conv = 5
    plan_refused(io, b"net[0].n_conv = 5")
    plan_refused(_io(L, with_(NOTEBOOK, convs=[(33, 1, 1, 1)]), None), b"net[0].conv_out[0] = 33")
    plan_refused(_io(L, with_(NOTEBOOK, convs=[(5, 5, 1, 1)]), None), b"net[0].conv_stride[0] = 5")
    plan_refused(_io(L, with_(NOTEBOOK, convs=[(5, 1, 9, 1)]), None), b"net[0].conv_padding[0] = 9")
    plan_refused(_io(L, with_(NOTEBOOK, convs=[(5, 1, 1, 5)]), None), b"net[0].conv_dilation[0] = 5")
    plan_refused(_io(L, with_(NOTEBOOK, N=2, k=5, convs=[(5, 1, 0, 1)]), None), b"net[0].conv layer 0", b"output size")
    plan_refused(_io(L, with_(NOTEBOOK, N=16, convs=[(32, 1, 1, 1)]), None), b"net[0].R = ", b"SUSNET_SPATIAL_MAX_R")  # R = 32 * 256 + 15
    plan_refused(_io(L, with_(NOTEBOOK, Fn=-1), None), b"net[0].Fn = -1")
    plan_refused(_io(L, with_(NOTEBOOK, layers=5), None), b"net[0].rnn_layers = 5")
    plan_refused(_io(L, with_(NOTEBOOK, hidden=257, dims=[257, 16, 5]), None), b"net[0].rnn_hidden = 257")
    plan_refused(_io(L, with_(NOTEBOOK, dims=[32, 16, 16, 5]), None), b"team[0].dims[0] = 32", b"rnn_hidden")
    plan_refused(_io(L, with_(NOTEBOOK, dims=[64]), None), b"team[0].n_dims")
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, dims=[64, 257, 5])), b"team[1].dims[1]", b"hidden")
    plan_refused(_io(L, with_(NOTEBOOK, dims=[64, 16, 33]), None), b"team[0].dims[2]", b"n_out")
    # teams that disagree on what they read
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, T=5)), b"net[1].T", b"both teams")
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, N=10)), b"net[1].N", b"both teams")
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, C=6)), b"net[1].C", b"both teams")
    plan_refused(_io(L, NOTEBOOK, with_(NOTEBOOK, Fn=14)), b"net[1].Fn", b"both teams")
    io = _io(L)
    io.team[1].packed = 4096
    plan_refused(io, b"team[1].packed")
    plan_refused(_io(L, n=-1), b"n = -1")
    plan_refused(_io(L, n=(1 << 30) + 1), b"n = ")
    io = _io(L)
    io.team[0].beta1 = 1.0
    plan_refused(io, b"team[0].", b"beta")
    io = _io(L)
    io.team[0].lr = -1e-3
    plan_refused(io, b"team[0].", b"lr")
    io = _io(L)
    io.spatial_stride[1] = -1
    plan_refused(io, b"spatial_stride[1] = -1")
    io = _io(L)
    io.non_spatial_stride[2] = -4
    plan_refused(io, b"non_spatial_stride[2] = -4")
    # pointers and the workspace: checked by the step
    for name in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        io = _io(L)
        setattr(io, name, None)
        refused(io, name.encode())
    for name in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "losses_out"):
        io = _io(L)
        setattr(io, name, 4098)
        refused(io, name.encode(), b"4-byte")
    for name in ("params", "target_params", "exp_avg", "exp_avg_sq", "step"):
        io = _io(L)
        setattr(io.team[1], name, None)
        refused(io, b"team[1]." + name.encode())
        setattr(io.team[1], name, 4097)
        refused(io, b"team[1]." + name.encode(), b"4-byte")
    io = _io(L)
    io.workspace = None
    refused(io, b"workspace")
    io = _io(L, workspace=(1 << 20) + 128)
    refused(io, b"workspace", b"256-byte aligned")
    io = _io(L)
    assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(io), C.byref(nbytes)) == 0
    io.workspace_bytes = nbytes.value - 1
    refused(io, b"workspace", b"smaller")
    io = _io(L)
    io.max_size = 0
    refused(io, b"max_size")
    assert lib.susnet_spatial_train_step(None, C.byref(_io(L)), None) == L.E_INVALID
    assert lib.susnet_spatial_train_step(h, None, None) == L.E_INVALID
    assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(_io(L)), None) == L.E_INVALID
    # Fn = 0: nothing is read through the non-spatial pointers, NULL passes the pointer checks (the refusal is the next one: the workspace)
    zero = with_(NOTEBOOK, Fn=0)
    io = _io(L, zero, zero)
    io.non_spatial = io.next_non_spatial = None
    io.workspace_bytes = 0
    refused(io, b"workspace")
    # a two-imposter handle: refused citing the reference line, as the other learners do
    h2 = _handle(L, lib, n_imposters=2, n_crew=3)
    plan_refused(_io(L), b"n_imposters", b"train.py:83", handle=h2)
    lib.susnet_destroy(h2)
    lib.susnet_destroy(h)


class _NoDevice:
    """What DeviceDQNTeamTrainer's recogniser needs of an env (SpatialQNet keeps a reference and reads nothing from it)."""


def test_the_recogniser_refuses_what_the_kernels_do_not_compute(pkg):
    """The trainer-level fall-backs (dropout between RNN layers, a FlatFeaturizer, a non-square kernel) on a device are in
    tests/test_gpu_spatial_train.py::test_unserved_trainers_fall_back (a trainer needs an env, an env a device); here the recogniser they rest on,
    and the default."""
    T = pkg.DeviceDQNTeamTrainer
    assert inspect.signature(T.__init__).parameters["spatial"].default is False
    tr = T.__new__(T)
    tr.env = _NoDevice()
    mk = lambda k, layers, dropout: pkg.SpatialDQN(9, 15, [7, 5, 3], [1, 1], [1, 1], k, [1, 1], layers, 16, dropout, [16], 5)
    with torch.random.fork_rng(devices=[]):
        good = tr._spatial_net(mk((3, 3), 2, 0.0))
        assert good is not None and good["convs"] == [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)] and good["dims"] == [16, 16, 5]
        assert tr._spatial_net(mk((3, 3), 1, 0.1)) is not None  # (nn.RNN drops out BETWEEN layers only: one layer has none)
        assert tr._spatial_net(mk((3, 3), 2, 0.1)) is None
        assert tr._spatial_net(mk((3, 1), 2, 0.0)) is None
        assert tr._spatial_net(pkg.MLP([4, 3])) is None
