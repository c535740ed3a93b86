"""The tables behind tests/test_spatial_desc_host.py and tests/golden/generate_spatial_refusals.py: what is asked (the cases) and how the
answers are taken (``record``), stated once so that the recording and the test cannot drift apart.  No device, no kernel: every C call
here is refused before anything is launched, every module is looked at on the host."""
import ctypes as C
import importlib

import torch
from torch import nn

# the notebook's network of tests/test_spatial_train_abi.py::NOTEBOOK
NOTEBOOK = dict(T=6, N=9, C=7, Fn=15, k=3, convs=[(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], layers=3, hidden=64, dims=[64, 16, 16, 5])
CONV_FIELDS = ("conv_out", "conv_stride", "conv_padding", "conv_dilation")


def _net(**over):
    """NOTEBOOK with fields replaced; ``conv_out=(l, v)`` (or a list of such pairs) replaces one layer's entry; ``n_conv`` / ``n_dims``
    override the counts the lists give."""
    d = dict(NOTEBOOK, convs=[list(c) for c in NOTEBOOK["convs"]], dims=list(NOTEBOOK["dims"]))
    for name, v in over.items():
        if name in CONV_FIELDS:
            for l, x in (v if isinstance(v, list) else [v]):
                d["convs"][l][CONV_FIELDS.index(name)] = x
        else:
            d[name] = v
    return d


# name: a network with ONE rule of susnet_spatial_forward / susnet_spatial_train_step violated
NET_VIOLATIONS = {}
for field, values in (("T", (0, 9)), ("N", (0, 17)), ("C", (0, 33)), ("n_conv", (0, 5)), ("k", (0, 2, 4, 7))):
    for v in values:
        NET_VIOLATIONS[f"{field}={v}"] = _net(**{field: v})
for field, l, values in (("conv_out", 1, (0, 33)), ("conv_stride", 2, (0, 5)), ("conv_padding", 0, (-1, 9)), ("conv_dilation", 1, (0, 5))):
    for v in values:
        NET_VIOLATIONS[f"{field}[{l}]={v}"] = _net(**{field: (l, v)})
NET_VIOLATIONS.update({
    "output_size<1": _net(N=1, k=5, conv_padding=(0, 1)),
    "Fn=-1": _net(Fn=-1),
    "R>4096": _net(N=16, conv_out=(2, 32)),
    "rnn_layers=0": _net(layers=0),
    "rnn_layers=5": _net(layers=5),
    "rnn_hidden=0": _net(hidden=0, dims=[0, 16, 16, 5]),
    "rnn_hidden=257": _net(hidden=257, dims=[257, 16, 16, 5]),
    "dims[0]!=rnn_hidden": _net(dims=[32, 16, 16, 5]),
    "n_dims=1": _net(dims=[64]),
    "n_dims=9": _net(dims=[64] + [16] * 6 + [5], n_dims=9),
    "dims[1]=257": _net(dims=[64, 257, 16, 5]),
    "last_dim=33": _net(dims=[64, 16, 16, 33]),
})

PTR = 4096  # plausible, aligned, never dereferenced


def handle(L, lib, n_imposters=1, n_crew=4):
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


def _fill_net(dst, d):
    """The fields susnet_spatial_io and susnet_spatial_net share."""
    dst.T, dst.N, dst.C, dst.Fn, dst.k, dst.n_conv = d["T"], d["N"], d["C"], d["Fn"], d["k"], d.get("n_conv", len(d["convs"]))
    for l, conv in enumerate(d["convs"][:4]):
        dst.conv_out[l], dst.conv_stride[l], dst.conv_padding[l], dst.conv_dilation[l] = conv
    dst.rnn_layers, dst.rnn_hidden = d["layers"], d["hidden"]


def _fill_dims(dst, d):
    dst.n_dims = d.get("n_dims", len(d["dims"]))
    for k, v in enumerate(d["dims"][:8]):
        dst.dims[k] = v


def forward_io(L, d=NOTEBOOK):
    io = L.SpatialIO()
    _fill_net(io, d)
    _fill_dims(io, d)
    for field, count in (("conv_weight", 4), ("conv_bias", 4), ("w_ih", 4), ("w_hh", 4), ("b_ih", 4), ("b_hh", 4), ("weight", 7), ("bias", 7), ("slope", 6)):
        for l in range(count):
            getattr(io, field)[l] = PTR
    io.spatial = io.non_spatial = io.rnn_in = io.q_out = PTR
    for k in range(3):
        io.spatial_stride[k] = io.non_spatial_stride[k] = 0
    io.agents, io.n = 5, 40
    return io


def _fill_team(tm, dims_of):
    tm.enabled = 1
    _fill_dims(tm, dims_of)
    tm.lr, tm.beta1, tm.beta2, tm.eps = 1e-3, 0.9, 0.999, 1e-8
    tm.params = tm.target_params = tm.exp_avg = tm.exp_avg_sq = tm.step = PTR


def spatial_train_io(L, net0=NOTEBOOK, net1=NOTEBOOK, n=5):
    io = L.SpatialTrainIO()
    for name in ("spatial", "next_spatial", "non_spatial", "next_non_spatial", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        setattr(io, name, PTR)
    io.max_size, io.n, io.gamma = 64, n, 0.9
    for t, d in enumerate((net0, net1)):
        _fill_team(io.team[t], d)
        _fill_net(io.net[t], d)
    io.workspace, io.workspace_bytes = 1 << 20, 1 << 40
    return io


MLP_DIMS = dict(dims=[36, 256, 128, 64, 16, 6])


def mlp_train_io(L, n=5):
    io = L.MlpTrainIO()
    for name in ("feat", "next_feat", "actions", "rewards", "dones", "imposters", "indices", "losses_out"):
        setattr(io, name, PTR)
    io.max_size, io.n, io.gamma = 64, n, 0.9
    for tm in io.team:
        _fill_team(tm, MLP_DIMS)
    io.workspace, io.workspace_bytes = 1 << 20, 1 << 40
    return io


def _set(path, value):
    def edit(io):
        obj = io
        *head, last = path.split(".")
        for part in head:
            obj = obj.team[int(part[5])] if part.startswith("team[") else getattr(obj, part)
        setattr(obj, last, value)
    return edit


# name: an edit of a well-formed learner io that violates ONE of the checks the dense and the spatial step share
LEARNER_VIOLATIONS = {"n=-1": _set("n", -1), "max_size=0": _set("max_size", 0), "team[0].beta1=1": _set("team[0].beta1", 1.0),
                      "team[1].lr<0": _set("team[1].lr", -1e-3), "workspace=NULL": _set("workspace", None),
                      "workspace_unaligned": _set("workspace", (1 << 20) + 128)}
for name in ("losses_out", "actions", "rewards", "dones", "imposters", "indices"):
    LEARNER_VIOLATIONS[f"{name}=NULL"] = _set(name, None)
LEARNER_VIOLATIONS["losses_out_misaligned"] = _set("losses_out", PTR + 2)
for name in ("params", "target_params", "exp_avg", "exp_avg_sq", "step"):
    LEARNER_VIOLATIONS[f"team[0].{name}=NULL"] = _set(f"team[0].{name}", None)
    LEARNER_VIOLATIONS[f"team[1].{name}_misaligned"] = _set(f"team[1].{name}", PTR + 1)

# entry: (the io's maker, its workspace query, whether it takes susnet_rnn_dropout structs)
LEARNERS = {"susnet_mlp_train_step": (mlp_train_io, "susnet_mlp_train_workspace_bytes", False),
            "susnet_spatial_train_step": (spatial_train_io, "susnet_spatial_train_workspace_bytes", False),
            "susnet_spatial_train_step_dropout": (spatial_train_io, "susnet_spatial_train_dropout_workspace_bytes", True)}


def _drop(L):
    drop = (L.RnnDropout * 2)()
    for d in drop:
        d.p[0] = d.p[1] = 0.2
        d.seed, d.offset, d.row_base = 7, 0, 0
    return drop


def record_refusals(pkg) -> dict:
    """Every refusal of the tables above as ``[return code, susnet_last_error()]``."""
    L = pkg._lib
    lib = L.lib()
    h, h2 = handle(L, lib), handle(L, lib, n_imposters=2, n_crew=3)
    nbytes = C.c_uint64()

    def said(rc):
        return [int(rc), lib.susnet_last_error().decode()]

    out = {"net": {}, "learner": {}}
    for name, d in NET_VIOLATIONS.items():
        team0, team1 = spatial_train_io(L, d, NOTEBOOK), spatial_train_io(L, NOTEBOOK, d)
        out["net"][name] = {
            "forward": said(lib.susnet_spatial_forward(h, C.byref(forward_io(L, d)), None)),
            "workspace_team0": said(lib.susnet_spatial_train_workspace_bytes(h, C.byref(team0), C.byref(nbytes))),
            "step_team0": said(lib.susnet_spatial_train_step(h, C.byref(team0), None)),
            "workspace_team1": said(lib.susnet_spatial_train_workspace_bytes(h, C.byref(team1), C.byref(nbytes))),
            "step_team1": said(lib.susnet_spatial_train_step(h, C.byref(team1), None)),
        }
    for entry, (make, query, drops) in LEARNERS.items():
        step = getattr(lib, entry)
        call = (lambda hh, io: step(hh, C.byref(io), _drop(L), None)) if drops else (lambda hh, io: step(hh, C.byref(io), None))
        rows = {}
        for name, edit in LEARNER_VIOLATIONS.items():
            io = make(L)
            edit(io)
            rows[name] = said(call(h, io))
        io = make(L)
        assert getattr(lib, query)(h, C.byref(io), C.byref(nbytes)) == 0, lib.susnet_last_error()
        io.workspace_bytes = nbytes.value - 1
        rows["workspace_one_byte_short"] = said(call(h, io))
        rows["two_imposters"] = said(call(h2, make(L)))
        out["learner"][entry] = rows
    lib.susnet_destroy(h2)
    lib.susnet_destroy(h)
    return out


# ---- the Python accept sets ----
def _dqn(pkg, **over):
    cfg = dict(input_image_size=9, non_spatial_input_size=8, n_channels=[5, 6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1],
               rnn_layers=2, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[16], n_actions=6)
    cfg.update(over)
    return pkg.policy.SpatialDQN(**cfg)


def modules(pkg) -> dict:
    """Hand-built SpatialDQNs: the three fixture networks (tests/golden/generate_spatial.py's two, generate_models.py's), then one rule each."""
    gru, bidir, prelu = _dqn(pkg), _dqn(pkg), _dqn(pkg)
    gru.rnn.model = nn.GRU(gru.rnn_in_dim, 16, 2, batch_first=True)
    bidir.rnn.model = nn.RNN(bidir.rnn_in_dim, 16, 2, batch_first=True, bidirectional=True)
    prelu.prediction_head[1] = nn.PReLU(16)
    return {
        "fixture_notebook": _dqn(pkg, non_spatial_input_size=15, n_channels=[7, 5, 3], rnn_layers=3, rnn_hidden_dim=64, mlp_hidden_layer_dims=[16, 16], n_actions=5),
        "fixture_perspective": _dqn(pkg, input_image_size=14, non_spatial_input_size=6, rnn_layers=1, mlp_hidden_layer_dims=[12], n_actions=5),
        "fixture_model_npz": _dqn(pkg, non_spatial_input_size=7, n_channels=[5, 8, 16], rnn_hidden_dim=32, mlp_hidden_layer_dims=[16, 8], n_actions=7),
        "kernel_3x1": _dqn(pkg, kernel_size=(3, 1)),
        "k=7": _dqn(pkg, kernel_size=(7, 7), paddings=[3, 3]),
        "five_convolutions": _dqn(pkg, n_channels=[5, 6, 7, 8, 9], strides=[1] * 4, paddings=[1] * 4, dilations=[1] * 4),
        "channels_33": _dqn(pkg, n_channels=[5, 6, 33]),
        "N=17": _dqn(pkg, input_image_size=17),
        "R>4096": _dqn(pkg, input_image_size=16, n_channels=[5, 6, 32]),
        "five_rnn_layers": _dqn(pkg, rnn_layers=5),
        "gru": gru,
        "bidirectional": bidir,
        "prelu_per_channel": prelu,
        "dropout_one_layer": _dqn(pkg, rnn_layers=1, rnn_dropout=0.2),
        "dropout_two_layers": _dqn(pkg, rnn_dropout=0.2),
        "hidden_256_two_layers": _dqn(pkg, rnn_hidden_dim=256),
    }


class NoDevice:
    """What the recognisers need of an env (``SpatialQNet`` keeps a reference and reads nothing from it) and, for the feed check, the shapes
    a featurizer's ``_make_obs`` buffers would have: planes ``[.., C, N, N]`` and ``Fn`` non-spatial columns (None: no such block)."""

    def __init__(self, n_agents=5, C=5, N=9, Fn=3):
        self.n_agents, self._shape = n_agents, (C, N, Fn)

    def _make_obs(self, config, ticks, rows=None):
        Cc, N, Fn = self._shape
        return None, torch.zeros(rows, Cc, N, N), (None if Fn is None else torch.zeros(rows, Fn))


NET_KEYS = ("N", "C", "Fn", "k", "convs", "layers", "hidden", "dims", "p")


def record_accepts(pkg) -> dict:
    """Per module: whether ``SpatialQNet`` declines it, the trainer's ``_spatial_net`` without and with dropout (its NET_KEYS, or None)
    and ``spatial_unserved_reason`` on a Global featurizer whose tensors are the default network's (5 channels, 9 x 9, 3 + 5 columns, 6 actions)."""
    T = pkg.trainer.DeviceDQNTeamTrainer
    env = NoDevice()
    tr = T.__new__(T)
    tr.env = env
    fz = pkg.features.GlobalFeaturizer(env)
    keys = lambda d: d and {k: (list(map(list, d[k])) if k == "convs" else d[k]) for k in NET_KEYS}
    out = {}
    with torch.random.fork_rng(devices=[]):
        for name, m in modules(pkg).items():
            out[name] = {"qnet_is_none": pkg.policy.SpatialQNet(env, m) is None, "trainer": keys(tr._spatial_net(m)),
                         "trainer_dropout": keys(tr._spatial_net(m, dropout=True)),
                         "unserved_reason": pkg.train_loop.spatial_unserved_reason(env, fz, m, 6, 2)}
        m = _dqn(pkg)
        out["reasons"] = {
            "not_a_spatial_dqn": pkg.train_loop.spatial_unserved_reason(env, fz, pkg.policy.MLP([4, 3]), 6, 2),
            "flat_featurizer": pkg.train_loop.spatial_unserved_reason(env, object(), m, 6, 2),
            "another_env": pkg.train_loop.spatial_unserved_reason(NoDevice(), fz, m, 6, 2),
            "T=9": pkg.train_loop.spatial_unserved_reason(env, fz, m, 6, 9),
            "no_non_spatial_block": pkg.train_loop.spatial_unserved_reason(*_with_env(pkg, NoDevice(Fn=None)), m, 6, 2),
            "other_channels": pkg.train_loop.spatial_unserved_reason(*_with_env(pkg, NoDevice(C=6)), m, 6, 2),
            "other_actions": pkg.train_loop.spatial_unserved_reason(env, fz, m, 5, 2),
            "perspective_width": pkg.train_loop.spatial_unserved_reason(env, pkg.features.PerspectiveFeaturizer(env), m, 6, 2),
        }
    return out


def _with_env(pkg, env):
    return env, pkg.features.GlobalFeaturizer(env)


def record() -> dict:
    pkg = importlib.import_module("sus-net_amd")
    return {"refusals": record_refusals(pkg), "accepts": record_accepts(pkg)}
