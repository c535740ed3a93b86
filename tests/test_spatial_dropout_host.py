"""CPU-only checks of dropout between the SpatialDQN's RNN layers in the train step: susnet_rnn_dropout against its ctypes mirror, the three
new symbols, the host-side refusals of the entry points (before any launch, on a handle without device buffers, naming the field), the float64
restatement of tests/spatial_dropout_util.py against the reference module's training-mode fixtures, and the Python defaults.  No kernel is
launched here."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from spatial_dropout_util import make_drop, masked_forward
from test_spatial_train_abi import NOTEBOOK, _handle, _io, _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("susnet_spatial_train_dropout_workspace_bytes", "susnet_spatial_train_step_dropout",
           "susnet_rnn_dropout_mask")
FIXTURES = ("l2_p50", "l3_p50", "l2_p20", "l3_p20")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_rnn_dropout_matches_the_header(pkg, tmp_path):
    L = pkg._lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(susnet_rnn_dropout));', 'printf("abi %d\\n", SUSNET_ABI_VERSION);',
             'printf("io_size %zu\\n", sizeof(susnet_spatial_io));', 'printf("train_io_size %zu\\n", sizeof(susnet_spatial_train_io));']
    for fname, _ in L.RnnDropout._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_rnn_dropout, {fname}));')
    lines += ["return 0;}"]
    prog = tmp_path / "rnn_dropout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "rnn_dropout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.RnnDropout) == 32
    for fname, _ in L.RnnDropout._fields_:
        assert int(out[fname]) == getattr(L.RnnDropout, fname).offset, fname
    assert int(out["abi"]) == 8 == L.ABI_VERSION  # additions only: the ABI version stays
    assert int(out["io_size"]) == C.sizeof(L.SpatialIO) and int(out["train_io_size"]) == C.sizeof(L.SpatialTrainIO)  # (neither grew)


def test_dropout_symbols_are_declared_exported_and_prototyped(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in pkg._lib.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int, s
    assert "#define SUSNET_ABI_VERSION 8" in header and lib.susnet_abi_version() == 8


def test_dropout_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    nbytes = C.c_uint64()

    def refused(rc, entry, *fields):
        msg = lib.susnet_last_error()
        assert rc == L.E_INVALID and entry in msg and all(f in msg for f in fields), (rc, fields, msg)

    bad_drops = [(dict(p_online=1.0), b"p[0]"), (dict(p_online=-0.1), b"p[0]"), (dict(p_online=float("nan")), b"p[0]"),
                 (dict(p_online=0.2, p_target=1.5), b"p[1]"), (dict(p_online=0.2, offset=1 << 56), b"offset"),
                 (dict(p_online=0.2, row_base=-1), b"row_base"), (dict(p_online=0.2, row_base=1 << 40), b"row_base")]
    # the mask export
    exp = b"susnet_rnn_dropout_mask"
    ok = dict(net=0, agent=0, layers=3, n=5, T=3, H=12)
    call = lambda drop, out=4096, **kw: lib.susnet_rnn_dropout_mask(h, drop, *[dict(ok, **kw)[k] for k in ("net", "agent", "layers", "n", "T", "H")], out, None)
    refused(call(None), exp, b"drop is NULL")
    for kw, field in bad_drops:
        refused(call(C.byref(make_drop(L, **kw))), exp, b"drop->", field)
    good = C.byref(make_drop(L, 0.2))
    for kw, field in ((dict(net=2), b"net = 2"), (dict(agent=4096), b"agent = 4096"), (dict(layers=1), b"layers = 1"), (dict(layers=5), b"layers = 5"),
                      (dict(n=0), b"n = 0"), (dict(T=9), b"T = 9"), (dict(H=257), b"H = 257"), (dict(H=0), b"H = 0")):
        refused(call(good, **kw), exp, field)
    refused(call(good, out=None), exp, b"out")
    refused(call(good, out=4098), exp, b"out", b"4-byte")
    # the train step: two structs, [0] imposters, [1] crew
    step = b"susnet_spatial_train_step_dropout"
    pair = lambda a, b: (L.RnnDropout * 2)(a, b)
    refused(lib.susnet_spatial_train_step_dropout(h, C.byref(_io(L)), None, None), step, b"drop is NULL")
    for kw, field in bad_drops:
        refused(lib.susnet_spatial_train_step_dropout(h, C.byref(_io(L)), pair(make_drop(L, 0.2), make_drop(L, **kw)), None), step, b"drop[1].", field)
        refused(lib.susnet_spatial_train_step_dropout(h, C.byref(_io(L)), pair(make_drop(L, **kw), make_drop(L, 0.2)), None), step, b"drop[0].", field)
    # (a team that is not enabled is not looked at: the refusal is the next one, the workspace)
    io = _io(L, NOTEBOOK, None)
    io.workspace = None
    refused(lib.susnet_spatial_train_step_dropout(h, C.byref(io), pair(make_drop(L, 0.2), make_drop(L, 7.0)), None), step, b"workspace")
    # everything the plain call refuses
    refused(lib.susnet_spatial_train_step_dropout(h, C.byref(_io(L, dict(NOTEBOOK, T=9), None)), pair(make_drop(L, 0.2), make_drop(L, 0.2)), None),
            step, b"net[0].T = 9")
    # the workspace: its own query, larger than the plain one by the multipliers' slices; the plain size is refused
    io = _io(L)
    assert lib.susnet_spatial_train_workspace_bytes(h, C.byref(io), C.byref(nbytes)) == 0
    plain = nbytes.value
    assert lib.susnet_spatial_train_dropout_workspace_bytes(h, C.byref(io), C.byref(nbytes)) == 0, lib.susnet_last_error()
    assert nbytes.value > plain and nbytes.value % 256 == 0
    io.workspace_bytes = plain
    refused(lib.susnet_spatial_train_step_dropout(h, C.byref(io), pair(make_drop(L, 0.2), make_drop(L, 0.2)), None), step, b"workspace",
            b"susnet_spatial_train_dropout_workspace_bytes")
    assert lib.susnet_spatial_train_dropout_workspace_bytes(h, C.byref(_io(L)), None) == L.E_INVALID
    assert lib.susnet_spatial_train_step_dropout(None, C.byref(_io(L)), pair(make_drop(L, 0.2), make_drop(L, 0.2)), None) == L.E_INVALID
    lib.susnet_destroy(h)


# ---- 2. the restatement against the reference's training-mode module ----------------------------------------------------------------------
def _load(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "spatial_dropout", name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files}


def fixture_model(pkg, meta, d):
    model = pkg.SpatialDQN(**meta["config"]).double()
    model.load_state_dict({k[len("param::"):]: torch.tensor(v) for k, v in d.items() if k.startswith("param::")})
    return model


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_in_training_mode(pkg, name):
    """tests/golden/generate_spatial_dropout.py: the unmodified reference SpatialDQN in training mode (float64, CPU), the masks torch drew.
    The restatement fed those masks gives its outputs -- and, for the case that has them, the gradients of a sum of gathered Q values --
    to 1e-12: this pins the restatement to the reference; the GPU tests pin the kernels to the restatement."""
    meta, d = _load(name)
    assert (meta["layers"], meta["p"]) == {"l2_p50": (2, 0.5), "l3_p50": (3, 0.5), "l2_p20": (2, 0.2), "l3_p20": (3, 0.2)}[name]
    model = fixture_model(pkg, meta, d)
    masks = [torch.tensor(m) for m in d["masks"]]
    s = 1.0 / (1.0 - meta["p"])
    assert len(masks) == meta["layers"] - 1 and all(bool(((m == 0) | (m == s)).all()) for m in masks)
    spatial, non_spatial = torch.tensor(d["spatial"]).double(), torch.tensor(d["non_spatial"]).double()
    q = masked_forward(model, spatial, non_spatial, masks)
    np.testing.assert_allclose(q.detach().numpy(), d["q"], rtol=0, atol=1e-12)
    assert float(np.abs(masked_forward(model, spatial, non_spatial, None).detach().numpy() - d["q"]).max()) > 1e-3, "the masks matter"
    grads = {k[len("grad::"):]: v for k, v in d.items() if k.startswith("grad::")}
    assert bool(grads) == (name == "l3_p50")
    if grads:
        torch.gather(q, 1, torch.tensor(d["actions"]).view(-1, 1)).sum().backward()
        for k, p in model.named_parameters():
            np.testing.assert_allclose(p.grad.numpy(), grads[k], rtol=0, atol=1e-12, err_msg=k)


# ---- 3. the Python defaults ------------------------------------------------------------------------------------------------------------------
def test_python_defaults_and_the_pinned_refusals(pkg):
    tl = pkg.train_loop
    for fn in (pkg.DeviceDQNTeamTrainer.__init__, tl.run_experiment):
        assert inspect.signature(fn).parameters["rnn_dropout_seed"].default is None, fn
    for fn in (tl.run_sweep, tl.evaluate, pkg.WindowedPolicyRollout.__init__):  # (acting has no dropout form: nothing to seed there)
        assert "rnn_dropout_seed" not in inspect.signature(fn).parameters
    T = pkg.DeviceDQNTeamTrainer
    tr = T.__new__(T)
    tr.env = _NoDevice()
    mk = lambda layers, hidden, head, dropout: pkg.SpatialDQN(9, 15, [7, 5, 3], [1, 1], [1, 1], (3, 3), [1, 1], layers, hidden, dropout, head, 5)
    with torch.random.fork_rng(devices=[]):
        # without the keyword: as before
        assert tr._spatial_net(mk(2, 16, [16], 0.1)) is None
        assert tr._spatial_net(mk(2, 16, [16], 0.1), dropout=False) is None
        # with it: the notebook's arguments (rnn_layers 3, rnn_dropout 0.2, 64 units, head [16, 16]) are served
        d = tr._spatial_net(mk(3, 64, [16, 16], 0.2), dropout=True)
        assert d is not None and (d["layers"], d["hidden"], d["dims"], d["p"]) == (3, 64, [64, 16, 16, 5], 0.2)
        assert tr._spatial_net(mk(1, 16, [16], 0.2), dropout=True)["p"] == 0.0  # (one layer: nothing to drop)
        # SpatialQNet still refuses a training-mode model with dropout between its layers: acting is the eval-mode forward
        m = mk(3, 64, [16, 16], 0.2)
        net = pkg.policy.SpatialQNet(_NoDevice(), m)
        with pytest.raises(RuntimeError, match="training mode"):
            net.forward(torch.zeros(1, 2, 7, 9, 9), torch.zeros(1, 2, 15))
