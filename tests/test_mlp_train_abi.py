"""CPU-only checks of the dense train step (susnet_mlp_train_step): the struct against its ctypes mirror, the two symbols, and the host-side
refusals -- every one before any launch, on a handle without device buffers, naming the field.  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("susnet_mlp_train_workspace_bytes", "susnet_mlp_train_step")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_mlp_train_io_matches_the_header(pkg, tmp_path):
    L = pkg._lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(susnet_mlp_train_io));', 'printf("team_size %zu\\n", sizeof(susnet_dqn_team));',
             'printf("abi %d\\n", SUSNET_ABI_VERSION);']
    for fname, _ in L.MlpTrainIO._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_mlp_train_io, {fname}));')
    lines += ["return 0;}"]
    prog = tmp_path / "mlp_train_io.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "mlp_train_io"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.MlpTrainIO)
    assert int(out["team_size"]) == C.sizeof(L.DqnTeam)
    for fname, _ in L.MlpTrainIO._fields_:
        assert int(out[fname]) == getattr(L.MlpTrainIO, fname).offset, fname
    assert int(out["abi"]) == 8 == L.ABI_VERSION  # additions only: the ABI version stays


def test_mlp_train_symbols_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in pkg._lib.EXPORTS and hasattr(lib, s), s
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8


def _handle(L, lib, n_imposters=1, n_crew=3):
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


GOOD = [36, 256, 128, 64, 16, 6]


def _io(L, dims0=GOOD, dims1=GOOD, n=5, ptr=4096, workspace=1 << 20):
    """A well-formed susnet_mlp_train_io whose pointers are plausible, aligned, never dereferenced values (every call below is refused)."""
    io = L.MlpTrainIO()
    for name in ("feat", "next_feat", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        setattr(io, name, ptr)
    io.max_size, io.n, io.gamma = 64, n, 0.9
    for tm, dims in zip(io.team, (dims0, dims1)):
        if dims is None:
            continue
        tm.enabled, tm.n_dims = 1, len(dims)
        for k, d in enumerate(dims[:8]):
            tm.dims[k] = d
        tm.lr, tm.beta1, tm.beta2, tm.eps = 1e-3, 0.9, 0.999, 1e-8
        tm.params = tm.target_params = tm.exp_avg = tm.exp_avg_sq = tm.step = ptr
    io.workspace, io.workspace_bytes = workspace, 1 << 40
    return io


def test_mlp_train_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound: the call needs none)
    nbytes = C.c_uint64()

    def refused(io, *fields, handle=h):
        assert lib.susnet_mlp_train_step(handle, C.byref(io), None) == L.E_INVALID, fields
        msg = lib.susnet_last_error()
        assert b"susnet_mlp_train_step" in msg and all(f in msg for f in fields), (fields, msg)

    def plan_refused(io, *fields, handle=h):
        """Refused by the workspace query too: the layer stack, n and the handle are checked there."""
        assert lib.susnet_mlp_train_workspace_bytes(handle, C.byref(io), C.byref(nbytes)) == L.E_INVALID, fields
        assert all(f in lib.susnet_last_error() for f in fields), (fields, lib.susnet_last_error())
        refused(io, *fields, handle=handle)

    # a well-formed io passes the plan (so every refusal below is about its one defect)
    assert lib.susnet_mlp_train_workspace_bytes(h, C.byref(_io(L)), C.byref(nbytes)) == 0, lib.susnet_last_error()
    assert nbytes.value > 0 and nbytes.value % 256 == 0
    for dims in ([4, 7], [8] * 8, [1024, 256, 32]):
        assert lib.susnet_mlp_train_workspace_bytes(h, C.byref(_io(L, dims, None)), C.byref(nbytes)) == 0, (dims, lib.susnet_last_error())
    plan_refused(_io(L, [36]), b"team[0].n_dims")
    plan_refused(_io(L, GOOD, [36, 8, 8, 8, 8, 8, 8, 8, 6]), b"team[1].n_dims")
    plan_refused(_io(L, [0] + GOOD[1:]), b"team[0].dims[0]")
    plan_refused(_io(L, [L.MLP_MAX_F + 1] + GOOD[1:], None), b"team[0].dims[0]", b"SUSNET_MLP_MAX_F")
    plan_refused(_io(L, [36, 256, 257, 64, 16, 6]), b"team[0].dims[2]", b"hidden")
    plan_refused(_io(L, GOOD, [36, 256, 128, 64, 16, 33]), b"team[1].dims[5]", b"n_out")
    plan_refused(_io(L, GOOD, [37] + GOOD[1:]), b"team[1].dims[0]", b"both teams")
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
    # pointers and the workspace: checked by the step
    for name in ("feat", "next_feat", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        io = _io(L)
        setattr(io, name, None)
        refused(io, name.encode())
    for name in ("params", "target_params", "exp_avg", "exp_avg_sq", "step"):
        io = _io(L)
        setattr(io.team[1], name, None)
        refused(io, b"team[1]." + name.encode())
    io = _io(L)
    io.feat = 4098
    refused(io, b"feat", b"4-byte")
    io = _io(L)
    io.workspace = None
    refused(io, b"workspace")
    io = _io(L, workspace=(1 << 20) + 128)
    refused(io, b"workspace", b"256-byte aligned")
    io = _io(L)
    assert lib.susnet_mlp_train_workspace_bytes(h, C.byref(io), C.byref(nbytes)) == 0
    io.workspace_bytes = nbytes.value - 1
    refused(io, b"workspace", b"smaller")
    io = _io(L)
    io.max_size = 0
    refused(io, b"max_size")
    assert lib.susnet_mlp_train_step(None, C.byref(_io(L)), None) == L.E_INVALID
    assert lib.susnet_mlp_train_step(h, None, None) == L.E_INVALID
    assert lib.susnet_mlp_train_workspace_bytes(h, C.byref(_io(L)), None) == L.E_INVALID
    # a two-imposter handle: refused citing the reference line, as susnet_dqn_train_step does
    h2 = _handle(L, lib, n_imposters=2, n_crew=3)
    plan_refused(_io(L), b"n_imposters", b"train.py:83", handle=h2)
    lib.susnet_destroy(h2)
    lib.susnet_destroy(h)


def test_workspace_respects_the_partial_cap(pkg):
    """The grid is capped so that all workgroups' partial gradients stay at or below 64 MiB: the workspace of the widest stack at the largest
    batch is bounded by lists + 64 MiB of partials + 256 slices of saved pre-activations."""
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    nbytes = C.c_uint64()
    wide = [1024, 256, 256, 256, 256, 256, 256, 32]
    n = 1 << 16
    assert lib.susnet_mlp_train_workspace_bytes(h, C.byref(_io(L, wide, wide, n=n)), C.byref(nbytes)) == 0, lib.susnet_last_error()
    P = sum(a * b + b for a, b in zip(wide[:-1], wide[1:])) + 6
    lists = 4 * 2 * 4 * n
    assert nbytes.value <= lists + (64 << 20) + 256 * 6 * 256 * 32 * 4 + 2 * 4 * (P + 4) + 8 * 256
    assert nbytes.value >= lists + 2 * 4 * P
    lib.susnet_destroy(h)
