"""CPU-only checks of the dense Q-network call (susnet_mlp_forward): the struct against its ctypes mirror, the host-side refusals (every
one before any launch, on a handle without device buffers) and which modules ``policy.DenseQNet`` serves.  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_mlp_io_matches_the_header(pkg, tmp_path):
    L = pkg._lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(susnet_mlp_io));']
    for fname, _ in L.MlpIO._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_mlp_io, {fname}));')
    lines += ['printf("max_f %d\\n", SUSNET_MLP_MAX_F);', 'printf("row_tile %d\\n", SUSNET_MLP_ROW_TILE);',
              'printf("max_grid %d\\n", SUSNET_MLP_MAX_GRID);', "return 0;}"]
    prog = tmp_path / "mlp_io.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "mlp_io"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.MlpIO)
    for fname, _ in L.MlpIO._fields_:
        assert int(out[fname]) == getattr(L.MlpIO, fname).offset, fname
    assert (int(out["max_f"]), int(out["row_tile"]), int(out["max_grid"])) == (L.MLP_MAX_F, L.MLP_ROW_TILE, L.MLP_MAX_GRID)
    assert L.MLP_MAX_F >= 1024
    # every flat layout of a 12-agent 14x14 game fits: all eight components together (component.py; csrc/susnet_obs.h flat_component_size)
    A, N, crew = 12, 14, 11
    assert A * 2 * N + 2 * A + (A - 1) + crew + crew + 9 + (A - 1) * 2 + 8 <= L.MLP_MAX_F


def test_mlp_forward_is_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    assert "susnet_mlp_forward" in declared and "susnet_mlp_forward" in pkg._lib.EXPORTS and hasattr(pkg._lib.lib(), "susnet_mlp_forward")
    assert "ascending" in header[header.index("CALLER-SUPPLIED"):header.index("typedef struct susnet_mlp_io")]  # the summation order is documented


def _handle(L, lib):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=8, n_imposters=1, n_crew=2, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                     shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


def _io(L, dims, n=5, ptr=4096):
    """A well-formed susnet_mlp_io whose pointers are plausible, aligned, never dereferenced values (the calls below are all refused)."""
    io = L.MlpIO()
    io.n_dims = len(dims)
    for k, d in enumerate(dims[:8]):
        io.dims[k] = d
    for l in range(7):
        io.weight[l], io.bias[l] = ptr, ptr
    for l in range(6):
        io.slope[l] = ptr
    io.rows, io.q_out, io.n = ptr, ptr, n
    return io


def test_mlp_forward_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound: the call needs none)
    good = [36, 256, 128, 64, 16, 6]

    def refused(io, field):
        assert lib.susnet_mlp_forward(h, C.byref(io), None) == L.E_INVALID, field
        msg = lib.susnet_last_error()
        assert b"susnet_mlp_forward" in msg and field in msg, (field, msg)

    refused(_io(L, [36]), b"n_dims")
    refused(_io(L, [36, 8, 8, 8, 8, 8, 8, 8, 6]), b"n_dims")
    refused(_io(L, [36, 256, 257, 64, 16, 6]), b"dims[2]")
    refused(_io(L, [36, 256, 128, 64, 16, 33]), b"dims[5]")
    assert b"n_out" in lib.susnet_last_error()
    refused(_io(L, [0] + good[1:]), b"dims[0]")
    refused(_io(L, [L.MLP_MAX_F + 1] + good[1:]), b"dims[0]")
    refused(_io(L, good, n=0), b"n = 0")
    io = _io(L, good)
    io.weight[3] = None
    refused(io, b"weight[3]")
    io = _io(L, good)
    io.rows = 4098
    refused(io, b"rows")
    io = _io(L, good)
    io.q_out = 4097
    refused(io, b"q_out")
    io = _io(L, good)
    io.slope[2] = None
    refused(io, b"slope[2]")
    assert lib.susnet_mlp_forward(None, C.byref(_io(L, good)), None) == L.E_INVALID
    assert lib.susnet_mlp_forward(h, None, None) == L.E_INVALID
    lib.susnet_destroy(h)


def test_dense_qnet_serves_reference_mlps_within_the_widths(pkg):
    P = pkg.policy
    spatial = P.SpatialDQN(input_image_size=9, non_spatial_input_size=8, n_channels=[5, 6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3),
                           dilations=[1, 1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[16], n_actions=6)
    assert P.DenseQNet(None, spatial) is None
    no_bias = P.MLP([37, 64, 7])
    no_bias.model[2] = nn.Linear(64, 7, bias=False)
    assert P.DenseQNet(None, no_bias) is None
    per_channel = P.MLP([37, 64, 7])
    per_channel.model[1] = nn.PReLU(64)
    assert P.DenseQNet(None, per_channel) is None
    assert P.DenseQNet(None, P.MLP([37, 300, 7])) is None
    assert P.DenseQNet(None, P.MLP([37, 64, 33])) is None
    assert P.DenseQNet(None, P.MLP([pkg._lib.MLP_MAX_F + 1, 64, 7])) is None
    assert P.DenseQNet(None, P.MLP([8] * 9)) is None  # eight Linear layers
    assert P.DenseQNet(None, nn.Linear(4, 7)) is None
    for dims in ([37, 200, 100, 50, 16, 7], [4, 7], [8] * 8):
        net = P.DenseQNet(None, P.MLP(dims))
        assert isinstance(net, P.DenseQNet) and net.dims == dims
