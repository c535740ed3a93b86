"""CPU-only checks of the SpatialDQN forward call (susnet_spatial_forward): the struct against its ctypes mirror, the host-side refusals
(every one before any launch, on a handle without device buffers), which modules ``policy.SpatialQNet`` serves, and the torch mirror
``policy.SpatialDQN`` against the reference outputs stored in tests/golden/spatial/*.npz.  No kernel is launched here."""
import ctypes as C
import glob
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPATIAL_DIR = os.path.join(ROOT, "tests", "golden", "spatial")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPATIAL_DIR, "*.npz")))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_spatial_io_matches_the_header(pkg, tmp_path):
    L = pkg._lib
    consts = {"max_t": "SUSNET_SPATIAL_MAX_T", "max_n": "SUSNET_SPATIAL_MAX_N", "max_c": "SUSNET_SPATIAL_MAX_C", "max_conv": "SUSNET_SPATIAL_MAX_CONV",
              "max_r": "SUSNET_SPATIAL_MAX_R", "max_rnn": "SUSNET_SPATIAL_MAX_RNN_LAYERS", "group": "SUSNET_SPATIAL_CONV_GROUP",
              "grid": "SUSNET_SPATIAL_CONV_MAX_GRID", "abi": "SUSNET_ABI_VERSION"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){", 'printf("size %zu\\n", sizeof(susnet_spatial_io));']
    for fname, _ in L.SpatialIO._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_spatial_io, {fname}));')
    lines += [f'printf("{k} %d\\n", {v});' for k, v in consts.items()] + ["return 0;}"]
    prog = tmp_path / "spatial_io.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "spatial_io"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.SpatialIO)
    for fname, _ in L.SpatialIO._fields_:
        assert int(out[fname]) == getattr(L.SpatialIO, fname).offset, fname
    got = tuple(int(out[k]) for k in consts)
    assert got == (L.SPATIAL_MAX_T, L.SPATIAL_MAX_N, L.SPATIAL_MAX_C, L.SPATIAL_MAX_CONV, L.SPATIAL_MAX_R, L.SPATIAL_MAX_RNN_LAYERS, L.SPATIAL_CONV_GROUP,
                   L.SPATIAL_CONV_MAX_GRID, L.ABI_VERSION)
    assert L.ABI_VERSION == 8  # an addition, as susnet_mlp_forward was


def test_spatial_forward_is_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    assert "susnet_spatial_forward" in declared and "susnet_spatial_forward" in pkg._lib.EXPORTS and hasattr(pkg._lib.lib(), "susnet_spatial_forward")
    doc = header[header.index("SpatialDQN.forward (src/models/dqn.py:205-301)"):header.index("typedef struct susnet_spatial_io")]
    for word in ("ascending", "EVAL", "dropout", "b_ih + b_hh", "Served", "dqn.py:141-181"):  # orders, eval-mode semantics, the served set
        assert word in doc, word


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


def _io(L, ptr=4096, **over):
    """A well-formed susnet_spatial_io (the notebook's network) whose pointers are plausible, aligned, never dereferenced values."""
    io = L.SpatialIO()
    io.T, io.N, io.C, io.n_conv, io.k, io.Fn = 6, 9, 7, 3, 3, 20
    for l, co in enumerate([5, 3, 3]):
        io.conv_out[l], io.conv_stride[l], io.conv_padding[l], io.conv_dilation[l] = co, 1, 1, 1
    io.rnn_layers, io.rnn_hidden, io.n_dims = 3, 64, 4
    for k, d in enumerate([64, 16, 16, 6]):
        io.dims[k] = d
    for field, count in (("conv_weight", 4), ("conv_bias", 4), ("w_ih", 4), ("w_hh", 4), ("b_ih", 4), ("b_hh", 4), ("weight", 7), ("bias", 7), ("slope", 6)):
        for l in range(count):
            getattr(io, field)[l] = ptr
    io.spatial = io.non_spatial = io.rnn_in = io.q_out = ptr
    for d, (a, b) in enumerate(((6 * 567, 6 * 5 * 20), (0, 20), (567, 5 * 20))):
        io.spatial_stride[d], io.non_spatial_stride[d] = a, b
    io.agents, io.n = 5, 40
    for name, v in over.items():
        if isinstance(v, list):
            for at, x in v:
                getattr(io, name)[at] = x
        elif isinstance(v, tuple):
            getattr(io, name)[v[0]] = v[1]
        else:
            setattr(io, name, v)
    return io


def test_spatial_forward_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound: the call needs none)

    def refused(field, **over):
        assert lib.susnet_spatial_forward(h, C.byref(_io(L, **over)), None) == L.E_INVALID, field
        msg = lib.susnet_last_error()
        assert b"susnet_spatial_forward" in msg and field in msg, (field, msg)

    for T in (0, 9):
        refused(b"T = ", T=T)
    for N in (0, 17):
        refused(b"N = ", N=N)
    for Cc in (0, 33):
        refused(b"C = ", C=Cc)
    for nc in (0, 5):
        refused(b"n_conv", n_conv=nc)
    for k in (0, 2, 4, 7):
        refused(b"k = ", k=k)
    for co in (0, 33):
        refused(b"conv_out[1]", conv_out=(1, co))
    for st in (0, 5):
        refused(b"conv_stride[2]", conv_stride=(2, st))
    for pd in (-1, 9):
        refused(b"conv_padding[0]", conv_padding=(0, pd))
    for dl in (0, 5):
        refused(b"conv_dilation[1]", conv_dilation=(1, dl))
    refused(b"output size", N=1, k=5, conv_padding=(0, 1))  # 1 + 2 - 4 - 1 < 0
    refused(b"Fn", Fn=-1)
    refused(b"R = ", N=16, conv_out=(2, 32))  # 32 * 256 + 20 > 4096
    for v in (0, 5):
        refused(b"rnn_layers", rnn_layers=v)
    for v in (0, 257):
        refused(b"rnn_hidden", rnn_hidden=v, dims=(0, v))
    for v in (1, 9):
        refused(b"n_dims", n_dims=v)
    refused(b"dims[0]", dims=(0, 32))
    refused(b"dims[1]", dims=(1, 257))
    refused(b"dims[3]", dims=(3, 33))
    assert b"n_out" in lib.susnet_last_error()
    refused(b"n = 0", n=0)
    refused(b"agents", agents=0)
    refused(b"spatial_stride[1]", spatial_stride=(1, -1))
    refused(b"non_spatial_stride[2]", non_spatial_stride=(2, -4))
    for field in ("conv_weight", "conv_bias", "w_ih", "w_hh", "b_ih", "b_hh", "weight", "bias", "slope"):
        refused(f"{field}[1]".encode(), **{field: (1, None)})
        refused(f"{field}[0]".encode(), **{field: (0, 4098)})
    for field in ("spatial", "non_spatial", "rnn_in", "q_out"):
        refused(field.encode(), **{field: None})
        refused(field.encode(), **{field: 4097})
    # Fn = 0: nothing is read through non_spatial, so NULL passes (a [B][T][0] tensor has no storage) and the strides are not looked at --
    # the call goes on to the NEXT check, which refuses the NULL workspace, so nothing is launched here; a misaligned pointer is still refused
    refused(b"rnn_in is NULL", Fn=0, non_spatial=None, rnn_in=None, non_spatial_stride=[(0, -1), (1, -1), (2, -1)])
    assert b"non_spatial" not in lib.susnet_last_error()
    refused(b"rnn_in is NULL", Fn=0, rnn_in=None)
    refused(b"non_spatial is NULL or not 4-byte aligned", Fn=0, non_spatial=4097)
    refused(b"non_spatial is NULL or not 4-byte aligned", Fn=1, non_spatial=None)
    refused(b"LDS", rnn_hidden=256, dims=(0, 256), rnn_layers=2)  # 3 x 64 x 256 floats = 192 KiB
    # one image: 32 KiB in, 32 x 32 x 32 floats = 128 KiB out of layer 0, 32 x 48 x 48 floats out of layer 1
    refused(b"LDS", C=32, N=16, k=1, conv_padding=[(0, 8), (1, 8)], conv_out=[(0, 32), (1, 32)], conv_stride=(2, 4))
    assert lib.susnet_spatial_forward(None, C.byref(_io(L)), None) == L.E_INVALID
    assert lib.susnet_spatial_forward(h, None, None) == L.E_INVALID
    lib.susnet_destroy(h)


def _load(path):
    z = np.load(path, allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _models_of(pkg, name):
    """``[(team, policy.SpatialDQN with the fixture's parameters, spatial, non_spatial, agents, want [B * agents, n])]``."""
    out = []
    if name == "model_spatialdqn":
        z, meta = _load(os.path.join(ROOT, "tests", "golden", "model_spatialdqn.npz"))
        m = pkg.policy.SpatialDQN(**meta["config"])
        m.load_state_dict({k: torch.from_numpy(z["param::" + k]) for k in meta["keys"]})
        return [("model", m.eval(), torch.from_numpy(z["input0"]), torch.from_numpy(z["input1"]), 1, torch.from_numpy(z["output"]))]
    z, meta = _load(os.path.join(SPATIAL_DIR, name + ".npz"))
    spatial, non_spatial = torch.from_numpy(z["spatial"].astype(np.float32)), torch.from_numpy(z["non_spatial"])
    for team in ("imposter", "crew"):
        m = pkg.policy.SpatialDQN(**dict(meta["config"], n_actions=meta["n_actions"][team]))
        m.load_state_dict({k[len(team) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(team + "::")})
        want = torch.from_numpy(z["q_" + team])
        out.append((team, m.eval(), spatial, non_spatial, spatial.shape[2], want.reshape(-1, want.shape[-1])))
    return out


def test_the_fixtures_are_there():
    assert FIXTURES == ["base14_1v2_persp_t3", "base_1v4_global_t6"]
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(SPATIAL_DIR, name + ".npz")) < 1 << 20


@pytest.mark.parametrize("name", ["model_spatialdqn", "base_1v4_global_t6", "base14_1v2_persp_t3"])
def test_spatial_qnet_serves_the_fixture_networks_and_the_mirror_reproduces_the_reference(pkg, name):
    for team, model, spatial, non_spatial, agents, want in _models_of(pkg, name):
        net = pkg.SpatialQNet(None, model)
        assert isinstance(net, pkg.SpatialQNet), (name, team)
        assert (net.C, net.N, net.Fn) == (spatial.shape[-3], spatial.shape[-1], non_spatial.shape[-1]) and net.R == model.rnn_in_dim
        with torch.no_grad():
            if spatial.dim() == 6:
                got = torch.stack([model(spatial[:, :, i], non_spatial[:, :, i]) for i in range(agents)], dim=1).reshape(want.shape)
            else:
                got = model(spatial, non_spatial)
        torch.testing.assert_close(got, want, rtol=0, atol=2e-5 * float(want.abs().max()))
        # every parameter matters: non-default slopes in the new fixtures
        if name != "model_spatialdqn":
            assert all(abs(float(m.weight.detach()) - 0.25) > 0.01 for m in model.prediction_head if isinstance(m, nn.PReLU))


def _spatial(pkg, **over):
    cfg = dict(input_image_size=9, non_spatial_input_size=8, n_channels=[5, 6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1],
               rnn_layers=2, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[16], n_actions=6)
    cfg.update(over)
    return pkg.policy.SpatialDQN(**cfg)


def test_spatial_qnet_declines_what_the_kernels_do_not_serve(pkg):
    P, Q = pkg.policy, pkg.SpatialQNet
    assert isinstance(Q(None, _spatial(pkg)), Q)
    assert P.DenseQNet(None, _spatial(pkg)) is None  # (stays true: the dense kernel serves MLPs)
    assert Q(None, P.MLP([37, 64, 7])) is None and Q(None, nn.Linear(4, 7)) is None
    m = _spatial(pkg)
    m.cnn.model[0] = nn.Conv2d(5, 6, kernel_size=(3, 1), padding=(1, 0))  # a non-square kernel
    assert Q(None, m) is None
    assert Q(None, _spatial(pkg, kernel_size=(7, 7), paddings=[3, 3])) is None
    for cls, kw in ((nn.GRU, {}), (nn.LSTM, {}), (nn.RNN, dict(nonlinearity="relu")), (nn.RNN, dict(bidirectional=True)), (nn.RNN, dict(bias=False))):
        m = _spatial(pkg)
        m.rnn.model = cls(m.rnn_in_dim, 16, num_layers=2, batch_first=True, **kw)
        assert Q(None, m) is None, (cls, kw)
    m = _spatial(pkg)
    m.prediction_head[1] = nn.PReLU(16)  # per-channel slopes
    assert Q(None, m) is None
    assert Q(None, _spatial(pkg, input_image_size=17)) is None
    assert Q(None, _spatial(pkg, n_channels=[33, 6, 8])) is None and Q(None, _spatial(pkg, n_channels=[5, 6, 33])) is None
    assert Q(None, _spatial(pkg, n_channels=[5, 6, 7, 8, 9], strides=[1] * 4, paddings=[1] * 4, dilations=[1] * 4)) is None  # five convolutions
    assert Q(None, _spatial(pkg, strides=[5, 5], paddings=[8, 8])) is None and Q(None, _spatial(pkg, paddings=[9, 9])) is None
    assert Q(None, _spatial(pkg, dilations=[5, 5], paddings=[8, 8])) is None
    assert Q(None, _spatial(pkg, input_image_size=16, n_channels=[5, 6, 32])) is None  # R = 32 * 256 + 8 > 4096
    assert Q(None, _spatial(pkg, rnn_layers=5)) is None and Q(None, _spatial(pkg, rnn_hidden_dim=257)) is None
    assert Q(None, _spatial(pkg, rnn_hidden_dim=256, rnn_layers=2)) is None  # the hidden-state buffers exceed a workgroup's LDS
    assert isinstance(Q(None, _spatial(pkg, rnn_hidden_dim=256, rnn_layers=1)), Q) and isinstance(Q(None, _spatial(pkg, rnn_hidden_dim=128, rnn_layers=4)), Q)
    assert Q(None, _spatial(pkg, mlp_hidden_layer_dims=[300])) is None and Q(None, _spatial(pkg, n_actions=33)) is None
    assert Q(None, _spatial(pkg, mlp_hidden_layer_dims=[8] * 7)) is None  # eight Linear layers


def test_spatial_qnet_refuses_training_mode_dropout(pkg):
    class Dev:  # what forward() reads of an env before the refusal
        device = torch.device("cpu")

    m = _spatial(pkg, rnn_dropout=0.5)
    net = pkg.SpatialQNet(Dev(), m)
    assert net is not None
    m.train()
    with pytest.raises(RuntimeError, match="dropout"):
        net.forward(torch.zeros(2, 2, 5, 9, 9), torch.zeros(2, 2, 8))


def test_torch_tanh_is_exact_where_the_exact_tests_need_it():
    x = torch.tensor([0.0, -0.0, 10.0, -10.0, 16.0, 32.0, -32.0, 64.0, -96.0, 3200.0])
    assert torch.equal(torch.tanh(x), torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0]))
