"""Policy-in-the-loop rollout (BASELINE.json config 5).

The loop around the HIP environment -- fused flat observation -> model -> argmax -> `step`, greedy as in the reference's
`run_game` (src/visualize.py:547-582) -- with every tensor staying on the device.  The networks are the reference's architectures
as torch modules (so that its checkpoints load); a reference ``MLP`` on one of the compiled-in feature layouts does not RUN through
torch, though: ``PolicyRollout`` hands its weights to the library once (``pack_mlp`` -> ``susnet_qnet_pack``) and a tick is then
one kernel (``susnet_qnet_policy_step``: network on the f32-input MFMA, argmax, the crew's draws, the env step), or two
(``susnet_qnet_forward`` + ``susnet_policy_step``) when the crew has a network too.  A reference ``MLP`` on any OTHER game, component
set or layer stack can run through the dense kernel (``PolicyRollout(..., dense=True)``: ``DenseQNet`` -> ``susnet_mlp_forward`` on
``env.obs``, weights read in place) and hand its Q rows to ``susnet_policy_step``: that is what ``collect`` / ``train`` / ``evaluate`` use
on those games.  By default, and for everything else (stacks wider than the dense kernel serves), the network runs
through stock PyTorch-ROCm -- which is the faster of the two at large batches -- and hands its Q rows to ``susnet_policy_step`` /
``susnet_policy_actions``.  ``PolicyRollout(..., dense=True, sequence_length=T)`` acts on the reference's WINDOW of the last T states
(train.py:318-322, 388-389, 441-445; ``run_experiment``'s default is T = 2): the policy keeps the window as feature rows ``[B, T * F]``,
``susnet_window_push`` moves it one tick on, and the dense kernel reads it as a row of width ``T * F`` (``MLP.forward`` flattens
``[B, T, F]`` the same way, dqn.py:86-90).

* ``MLP`` mirrors reference src/models/dqn.py:72-108 (`make_mlp` 322-329: Linear + PReLU, last activation
  dropped) INCLUDING the module names, so a reference checkpoint `{"state_dict", "config"}`
  (dqn.py:92-103) loads unchanged.  The reference ships no checkpoints (`.gitignore:2`), so benchmarks use a
  seeded random initialisation of the same architecture (layer dims of notebooks/experiment_1v1.ipynb cell 1).
* ``RandomEquiprobable`` mirrors dqn.py:111-138; in the loop a random crew is sampled by the environment's own
  `sample_actions` kernel (uniform over the role-valid indices, base.py:326-330).
* ``SpatialDQN`` mirrors dqn.py:205-314 (CNN over the plane features of every window step -> concat with the
  non-spatial features -> RNN over the window -> PReLU MLP head on the last hidden state), again with the reference's
  module names and its layer-list quirks, so reference checkpoints load; ``tests/golden/model_spatialdqn.npz`` pins it
  against the reference module's own forward pass.
* ``WindowedPolicyRollout`` is the batched form of the reference's acting loop with a state window
  (train.py:316-389, visualize.py:502-585): a ``[B, T, S]`` window of flattened states lives on the device, every
  tick it goes through ``susnet_featurize`` (Perspective / Global / Flat featurizer), each agent's view feeds the
  imposter or the crew network by the env's role mask, argmax (optionally epsilon-greedy, train.py:355-381), step,
  window roll (np.roll, train.py:388-389) or refill with the fresh first state where an episode ended.  With ``kernels=True`` a
  served ``SpatialDQN`` runs through ``SpatialQNet`` -> ``susnet_spatial_forward`` (convolutions on the vector ALU, recurrence and head on
  the f32-input MFMA), one call per team per tick for all ``B * A`` rows.  What a served ``SpatialDQN`` is, whether a featurizer feeds it
  and how raw rows become the kernels' inputs is stated once, for the actor and the trainer: ``spatial_desc``, ``spatial_feed_mismatch``,
  ``SpatialFeed``.
"""
from __future__ import annotations

import ctypes as C
from functools import cached_property, partial
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib as L
from .env import ObsConfig


def make_mlp(layer_dims: Sequence[int]) -> nn.Sequential:  # dqn.py:322-329 with PReLU (dqn.py:79)
    layers: List[nn.Module] = []
    for idx, dim in enumerate(layer_dims[:-1]):
        layers.append(nn.Linear(in_features=dim, out_features=layer_dims[idx + 1]))
        layers.append(nn.PReLU())
    return nn.Sequential(*layers[:-1])


class MLP(nn.Module):
    def __init__(self, layer_dims):
        super().__init__()
        self.layer_dims = list(layer_dims)
        self.model = make_mlp(self.layer_dims)
        self.config = {"layer_dims": self.layer_dims}

    def forward(self, spatial_x, non_spatial_x):  # dqn.py:84-88: the spatial input is ignored
        batch_size = spatial_x.size(0)
        return self.model(non_spatial_x.reshape(batch_size, -1))

    def dump_to_checkpoint(self, filepath):  # dqn.py:90-93
        torch.save({"state_dict": self.state_dict(), "config": self.config}, filepath)

    @staticmethod
    def load_from_checkpoint(filepath, map_location=None):  # dqn.py:95-101
        checkpoint = torch.load(filepath, map_location=map_location)
        model = MLP(**checkpoint["config"])
        model.load_state_dict(checkpoint["state_dict"])
        return model

    def create_copy(self):
        new = MLP(**self.config)
        new.load_state_dict(self.state_dict())
        return new


class RandomEquiprobable(nn.Module):  # dqn.py:111-138
    def __init__(self, n_outputs: int):
        super().__init__()
        self.n_outputs = n_outputs

    def forward(self, *inputs):
        batch = inputs[0].shape[0] if inputs else 1
        dev = inputs[0].device if inputs else None
        idx = torch.randint(0, self.n_outputs, (batch,), device=dev)
        out = torch.zeros(batch, self.n_outputs, device=dev)
        out[torch.arange(batch, device=dev), idx] = 1
        return out


def calculate_cnn_output_dim(input_size, kernel_size, strides, paddings, dilations):  # src/utils.py:5-11
    size = input_size
    for stride, padding, dilation in zip(strides, paddings, dilations):
        size = (size + 2 * padding - dilation * (kernel_size[0] - 1) - 1) // stride + 1
    return size


class _CNN(nn.Module):  # dqn.py:141-181; attribute name `model` = the checkpoint key prefix "cnn.model."
    def __init__(self, n_channels, strides, paddings, kernel_size, dilations):
        super().__init__()
        # the reference repeats the LAST entry of every list once more and zips them: with len(n_channels) ==
        # len(strides) + 1 that appends one extra same-width convolution (dqn.py:155-159)
        chans = list(n_channels) + [n_channels[-1]]
        strides, paddings, dilations = (list(v) + [v[-1]] for v in (strides, paddings, dilations))
        layers: List[nn.Module] = []
        for idx, (c_in, stride, padding, dilation) in enumerate(zip(chans[:-1], strides, paddings, dilations)):
            layers += [nn.Conv2d(c_in, chans[idx + 1], kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation),
                       nn.ReLU()]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


class _RNN(nn.Module):  # dqn.py:184-202
    def __init__(self, input_dim, n_layers, hidden_dim, dropout):
        super().__init__()
        self.model = nn.RNN(input_size=input_dim, hidden_size=hidden_dim, num_layers=n_layers, dropout=dropout, batch_first=True)

    def forward(self, x):
        return self.model(x)


class SpatialDQN(nn.Module):
    def __init__(self, input_image_size, non_spatial_input_size, n_channels, strides, paddings, kernel_size, dilations,
                 rnn_layers, rnn_hidden_dim, rnn_dropout, mlp_hidden_layer_dims, n_actions):
        super().__init__()
        self.config = dict(input_image_size=input_image_size, non_spatial_input_size=non_spatial_input_size,
                           n_channels=list(n_channels), strides=list(strides), paddings=list(paddings), dilations=list(dilations),
                           kernel_size=kernel_size, rnn_layers=rnn_layers, rnn_hidden_dim=rnn_hidden_dim, rnn_dropout=rnn_dropout,
                           mlp_hidden_layer_dims=list(mlp_hidden_layer_dims), n_actions=n_actions)
        self.cnn_ouput_dim = calculate_cnn_output_dim(input_image_size, kernel_size, strides, paddings, dilations)  # (sic)
        self.cnn = _CNN(n_channels, strides, paddings, kernel_size, dilations)
        self.rnn_in_dim = self.cnn_ouput_dim ** 2 * n_channels[-1] + non_spatial_input_size
        self.rnn = _RNN(self.rnn_in_dim, rnn_layers, rnn_hidden_dim, rnn_dropout)
        self.n_actions = n_actions
        self.mlp_dims = [rnn_hidden_dim] + list(mlp_hidden_layer_dims) + [n_actions]
        self.prediction_head = make_mlp(self.mlp_dims)

    def forward(self, spatial_x, non_spatial_x):  # dqn.py:275-293
        batch, steps, C, H, W = spatial_x.shape
        feats = self.cnn(spatial_x.reshape(batch * steps, C, H, W)).reshape(batch, steps, -1)
        out, _ = self.rnn(torch.cat((feats, non_spatial_x), dim=2))
        return self.prediction_head(out[:, -1, :])

    def dump_to_checkpoint(self, filepath):  # dqn.py:295-298
        torch.save({"state_dict": self.state_dict(), "config": self.config}, filepath)

    @staticmethod
    def load_from_checkpoint(filepath, map_location=None):  # dqn.py:300-306
        checkpoint = torch.load(filepath, map_location=map_location)
        model = SpatialDQN(**checkpoint["config"])
        model.load_state_dict(checkpoint["state_dict"])
        return model

    def create_copy(self):
        new = SpatialDQN(**self.config)
        new.load_state_dict(self.state_dict())
        return new


def reference_imposter_mlp(env, components: Sequence[str], seed: int = 0) -> MLP:
    """`[F, 256, 128, 64, 16, n_imposter_actions]` (notebooks/experiment_1v1.ipynb cell 1), seeded init."""
    spec, o1, _ = env._make_obs(ObsConfig("flat", list(components)), 1)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = MLP([o1.shape[-1], 256, 128, 64, 16, env.n_imposter_actions])
    return model.to(env.device).eval()


def reference_crew_mlp(env, components: Sequence[str], seed: int = 1) -> MLP:
    """The crew's network of the same architecture, `[F, 256, 128, 64, 16, n_crew_actions]` (train_crew, notebooks/experiment.ipynb cell 5;
    run_game's crew_model, visualize.py:547-562), seeded init."""
    spec, o1, _ = env._make_obs(ObsConfig("flat", list(components)), 1)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = MLP([o1.shape[-1], 256, 128, 64, 16, env.n_crew_actions])
    return model.to(env.device).eval()


def linear_prelu_stack(layers, chained: bool = True, trailing_act: bool = False):
    """``(linears, activations, dims = [in, out_1, .., out_n])`` of a layer list that is ``make_mlp``'s stack (dqn.py:322-329) -- ``Linear(bias=True)``
    and single-slope ``nn.PReLU`` alternating, none after the last Linear, the widths chained -- or None: what ``pack_mlp``, ``DenseQNet``,
    ``SpatialQNet``'s head and the dense learner accept.  ``chained=False`` / ``trailing_act=True`` give a second, wider accept set, that of
    ``DeviceDQNTeamTrainer._mlp_dims`` alone, which has never asked for either condition (see there)."""
    layers = list(layers)
    linears, acts = layers[0::2], layers[1::2]
    if not linears or not (len(acts) == len(linears) - 1 or (trailing_act and len(acts) == len(linears))) or \
            not all(isinstance(m, nn.Linear) and m.bias is not None for m in linears) or \
            not all(isinstance(m, nn.PReLU) and m.weight.numel() == 1 for m in acts) or \
            (chained and any(a.out_features != b.in_features for a, b in zip(linears[:-1], linears[1:]))):
        return None
    return linears, acts, [linears[0].in_features] + [m.out_features for m in linears]


def stack_within_bounds(dims, max_in: Optional[int] = None) -> bool:
    """Whether ``dims[1:]`` is what the dense kernels serve (``susnet_mlp_forward``, ``susnet_spatial_forward``'s head, ``susnet_mlp_train_step``:
    at most 7 Linear layers, hidden widths 1 .. ``MLP_MAX_HIDDEN``, 1 .. ``MLP_MAX_OUT`` outputs) and, with ``max_in``, ``dims[0]`` is in
    1 .. ``max_in``.  The C side of the same statement: ``check_stack_dims`` (csrc/susnet_host.h)."""
    return len(dims) - 1 <= 7 and (max_in is None or 1 <= dims[0] <= max_in) and all(1 <= d <= L.MLP_MAX_HIDDEN for d in dims[1:-1]) and \
        1 <= dims[-1] <= L.MLP_MAX_OUT


def _mlp_stack(model):
    """``linear_prelu_stack`` of a reference ``MLP``, or None."""
    return linear_prelu_stack(model.model) if isinstance(model, MLP) else None


def dense_stack(model):
    """``_mlp_stack`` within the dense kernels' bounds (``DenseQNet`` acts with it, ``DeviceDQNTeamTrainer(dense=True)`` trains it), or None."""
    stack = _mlp_stack(model)
    return stack if stack is not None and stack_within_bounds(stack[2], L.MLP_MAX_F) else None


def pack_mlp(env, model, components: Sequence[str], into=None):
    """``env.qnet_pack`` of a reference ``MLP`` (Linear / nn.PReLU() alternating, dqn.py:322-329), or None if ``model`` is something
    else or the library does not serve its shape on this env.  ``into``: an image of the same stack to overwrite in place."""
    stack = _mlp_stack(model)  # (widths that do not chain were left to env.qnet_pack, which returns None for them: the same answer, sooner)
    if stack is None:
        return None
    linears, acts, _ = stack
    cpu = lambda t: t.detach().to("cpu", torch.float32).numpy()
    return env.qnet_pack(components, [cpu(m.weight) for m in linears], [cpu(m.bias) for m in linears], [float(m.weight.detach()) for m in acts], into=into)


def _param_ptr(device, who: str, p) -> int:
    """``data_ptr()`` of a parameter the kernels read in place (``who``: the wrapper class, for the message)."""
    if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError(f"{who}: the model's parameters must be contiguous float32 tensors on {device} (got {p.dtype} on {p.device})")
    return p.data_ptr()


def fill_stack(io, linears, acts, ptr) -> None:
    """``n_dims / dims / weight / bias / slope`` of an io struct (``MlpIO``, ``SpatialIO``: the same field names) from a recognised stack."""
    io.n_dims = len(linears) + 1
    io.dims[0] = linears[0].in_features
    for l, m in enumerate(linears):
        io.dims[l + 1], io.weight[l], io.bias[l] = m.out_features, ptr(m.weight), ptr(m.bias)
    for l, m in enumerate(acts):
        io.slope[l] = ptr(m.weight)


def _out_rows(net, out, n: int, device):
    """Where a wrapper's Q rows ``[n, n_out]`` go: the caller's ``out``, checked, or the buffer ``net`` owns (``net._q``, re-made when ``n`` changes)."""
    n_out = net.dims[-1]
    if out is None:
        out = net._q
        if out is None or out.shape[0] != n:
            out = net._q = torch.empty(n, n_out, dtype=torch.float32, device=device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, n_out) and out.is_contiguous() and out.device == device
    return out


def window_push_reference(src, fresh, done=None, truncated=None):
    """``susnet_window_push`` restated in torch (or numpy) ops, on any device: the window ``src [n, T * F]`` one tick on with the fresh
    rows ``fresh [n, F]`` -- ``fresh`` repeated T times where ``done | truncated`` (train.py:441-445), else ``src[:, F:] ++ fresh``
    (train.py:388-389).  float32 tensors are moved as int32 bit patterns, as the kernel moves them.  Returns a new array."""
    n, F = fresh.shape
    T = src.shape[1] // F
    assert src.shape == (n, T * F), f"src is [n, T * F] = [{n}, T * {F}], got {tuple(src.shape)}"
    if isinstance(src, torch.Tensor):
        bits = src.dtype == torch.float32
        s, f = (src.view(torch.int32), fresh.view(torch.int32)) if bits else (src, fresh)
        ended = torch.zeros(n, dtype=torch.bool, device=src.device)
        for flag in (done, truncated):
            if flag is not None:
                ended = ended | flag.reshape(n).to(torch.bool)
        out = torch.where(ended.view(n, 1), f.repeat(1, T), torch.cat([s[:, F:], f], 1)).contiguous()
        return out.view(torch.float32) if bits else out
    import numpy as np

    bits = src.dtype == np.float32
    s, f = (src.view(np.int32), fresh.view(np.int32)) if bits else (src, fresh)
    ended = np.zeros(n, dtype=bool)
    for flag in (done, truncated):
        if flag is not None:
            ended |= np.asarray(flag).reshape(n).astype(bool)
    out = np.ascontiguousarray(np.where(ended[:, None], np.tile(f, (1, T)), np.concatenate([s[:, F:], f], 1)))
    return out.view(np.float32) if bits else out


class DenseQNet:
    """A reference ``MLP`` served by ``susnet_mlp_forward``: ``MLP.forward`` (dqn.py:72-108) as one HIP kernel on feature rows in device
    memory -- any game, component set and layer stack within the kernel's widths (1..7 ``Linear(bias=True)`` layers with single-slope
    ``PReLU``s between them, input width up to ``_lib.MLP_MAX_F``, hidden widths up to 256, at most 32 outputs).  ``DenseQNet(env, model)``
    is None for anything else (callers then run the torch module).

    Nothing is packed and nothing is cached: every ``forward`` takes the parameter tensors' ``data_ptr()``s afresh, so in-place updates
    (``optimizer.step``, ``load_state_dict``, ``susnet_dqn_train_step`` on a flat buffer) AND re-pointed parameters (the trainer moves
    ``p.data`` into its flat buffer) are followed without a refresh.  The one limit: a captured graph freezes the pointers it was captured
    with -- a replay follows in-place updates, not re-pointing (capture after the trainer is built)."""

    def __new__(cls, env, model):
        stack = dense_stack(model)
        if stack is None:
            return None
        self = super().__new__(cls)
        self.env, self.model = env, model
        self._linears, self._acts, self.dims = stack
        self._q = None  # the [rows][n_out] output buffer this object owns: the one of the most recent row count
        return self

    @torch.no_grad()
    def forward(self, rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Q rows ``[n, n_out]`` of ``rows`` (``[n, F]`` float32 contiguous on the env's device; default: ``env.obs``, the fused flat
        observation).  ``out``: where they go (default: the buffer this object keeps, re-made when ``n`` changes: a result is valid until
        the next call).  One launch, asynchronous."""
        env = self.env
        if rows is None:
            rows = env.obs
        F = self.dims[0]
        assert rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == F and rows.is_contiguous() and rows.device == env.device, (
            f"DenseQNet: rows must be a contiguous float32 [n, {F}] tensor on {env.device}")
        n = rows.shape[0]
        out = _out_rows(self, out, n, env.device)
        io = L.MlpIO()
        fill_stack(io, self._linears, self._acts, partial(_param_ptr, env.device, "DenseQNet"))
        io.rows, io.n, io.q_out = rows.data_ptr(), n, out.data_ptr()
        with env._on_device():
            L.check(env.lib.susnet_mlp_forward(env._h, C.byref(io), env._stream()))
        return out


def _spatial_stack(model):
    """What ``susnet_spatial_forward`` needs to know of a ``SpatialDQN`` -- ``dict(convs, k, rnn, head linears, head activations, head dims)`` -- or
    None if the module is something else or has a part the kernels do not compute."""
    if not isinstance(model, SpatialDQN):
        return None
    layers = list(model.cnn.model)
    convs, relus = layers[0::2], layers[1::2]
    if not convs or len(relus) != len(convs) or not all(isinstance(m, nn.Conv2d) and m.bias is not None for m in convs) or \
            not all(isinstance(m, nn.ReLU) for m in relus):
        return None
    same = lambda v: len(set(v)) == 1
    for m in convs:
        if not (same(m.kernel_size) and same(m.stride) and same(m.dilation)) or isinstance(m.padding, str) or not same(m.padding) or \
                m.groups != 1 or m.padding_mode != "zeros" or m.kernel_size != convs[0].kernel_size:
            return None
    if any(a.out_channels != b.in_channels for a, b in zip(convs[:-1], convs[1:])):
        return None
    rnn = model.rnn.model
    if not isinstance(rnn, nn.RNN) or rnn.mode != "RNN_TANH" or rnn.bidirectional or not rnn.bias or not rnn.batch_first or \
            getattr(rnn, "proj_size", 0) != 0:
        return None
    head = linear_prelu_stack(model.prediction_head)
    if head is None or head[0][0].in_features != rnn.hidden_size:
        return None
    return dict(convs=convs, k=convs[0].kernel_size[0], rnn=rnn, linears=head[0], acts=head[1], dims=head[2])


def spatial_desc(model):
    """The ONE description of a ``SpatialDQN`` the spatial kernels serve, or None: ``_spatial_stack`` within every bound of ``include/susnet.h``
    (the C side of the same statement: ``check_spatial_net``, csrc/susnet_host.h) and the two LDS sizes (``spatial_conv_lds`` /
    ``spatial_rnn_lds``, csrc/inst_qnet_spatial.hip).  ``dict(N, C, Fn, k, convs = [(out, stride, padding, dilation)], sizes = [N, layer
    outputs ..], R, layers, hidden, linears, acts, dims, p)`` -- ``p`` the dropout between RNN layers (0.0 with one layer) -- and the modules
    whose parameters are read in place (``conv_modules``, ``rnn``).  ``SpatialQNet`` acts with it, ``DeviceDQNTeamTrainer`` trains it."""
    stack = _spatial_stack(model)
    if stack is None:
        return None
    modules, k, rnn, dims = stack["convs"], stack["k"], stack["rnn"], stack["dims"]  # (dims[0] is rnn.hidden_size)
    N, C, Fn = int(model.config["input_image_size"]), modules[0].in_channels, int(model.config["non_spatial_input_size"])
    if k not in (1, 3, 5) or not 1 <= len(modules) <= L.SPATIAL_MAX_CONV or not 1 <= N <= L.SPATIAL_MAX_N or not 1 <= C <= L.SPATIAL_MAX_C or Fn < 0:
        return None
    convs, sizes = [(m.out_channels, m.stride[0], m.padding[0], m.dilation[0]) for m in modules], [N]
    for out, stride, padding, dilation in convs:
        span = sizes[-1] + 2 * padding - dilation * (k - 1) - 1
        if not (1 <= out <= 32 and 1 <= stride <= 4 and 0 <= padding <= 8 and 1 <= dilation <= 4) or span < 0:
            return None
        sizes.append(span // stride + 1)
    R, layers = convs[-1][0] * sizes[-1] ** 2 + Fn, rnn.num_layers
    if R != rnn.input_size or R > L.SPATIAL_MAX_R or not 1 <= layers <= L.SPATIAL_MAX_RNN_LAYERS or \
            not stack_within_bounds(dims, L.MLP_MAX_HIDDEN):  # (the head's input is the hidden state: rnn_hidden in 1 .. 256)
        return None
    slots = [C * N * N, 0]  # the convolution kernel's two LDS buffers per image (layer l writes buffer 1 - l % 2) ...
    for l, (out, *_) in enumerate(convs[:-1]):
        slots[1 - (l & 1)] = max(slots[1 - (l & 1)], out * sizes[l + 1] ** 2)
    # ... and the recurrence's rotating hidden buffers
    if 4 * sum(slots) > L.SPATIAL_LDS_BYTES or 4 * (layers + 1) * L.MLP_ROW_TILE * max(dims[:-1]) > L.SPATIAL_LDS_BYTES:
        return None
    return dict(N=N, C=C, Fn=Fn, k=k, convs=convs, sizes=sizes, R=R, layers=layers, hidden=rnn.hidden_size, linears=stack["linears"],
                acts=stack["acts"], dims=dims, p=float(rnn.dropout) if layers > 1 else 0.0, conv_modules=modules, rnn=rnn)


def fill_spatial_net(dst, desc, T: int) -> None:
    """The network's shape in a ``SpatialIO`` or a ``SpatialNet`` (the same field names) from a ``spatial_desc``, as ``fill_stack`` does for the head."""
    dst.T, dst.N, dst.C, dst.Fn, dst.n_conv, dst.k = T, desc["N"], desc["C"], desc["Fn"], len(desc["convs"]), desc["k"]
    for l, conv in enumerate(desc["convs"]):
        dst.conv_out[l], dst.conv_stride[l], dst.conv_padding[l], dst.conv_dilation[l] = conv
    dst.rnn_layers, dst.rnn_hidden = desc["layers"], desc["hidden"]


def spatial_feed_mismatch(env, featurizer, desc, n_actions: int) -> Optional[str]:
    """Why the tensors of ``featurizer`` (Global / Perspective, over ``env``) do not feed the network of ``desc`` with ``n_actions`` outputs, or
    None if they do: the actor, the trainer and ``train_loop.spatial_unserved_reason`` ask here."""
    from .features import GlobalFeaturizer

    # the featurizer's own shapes: planes [.., C, N, N]; non-spatial columns per agent view (the Global featurizer appends onehot(agent))
    _, planes, non_spatial = env._make_obs(featurizer.config, 1, rows=1)
    if non_spatial is None:  # (forward() takes a real non_spatial tensor)
        return "the featurizer has no non-spatial block"
    Fn = non_spatial.shape[-1] + (env.n_agents if isinstance(featurizer, GlobalFeaturizer) else 0)
    reads, want = (desc["C"], desc["N"], desc["Fn"], desc["dims"][-1]), (planes.shape[-3], planes.shape[-1], Fn, n_actions)
    if reads != want:
        return f"the network reads (channels, image size, non-spatial width, actions) = {reads}, the featurizer and the game give {want}"
    return None


def spatial_strides(x, inner: int, agents: int, what: str):
    """(env, agent, timestep) strides in floats of ``x``: ``[B, T, A, *inner]`` (a view per agent) or ``[B, T, *inner]`` (one for all)."""
    per_agent = x.dim() == inner + 3
    assert x.dim() in (inner + 2, inner + 3) and x.dtype == torch.float32, f"SpatialQNet: {what} is float32 [B, T, (A,) ...], got {tuple(x.shape)} {x.dtype}"
    tail = x.shape[-inner:]
    want, expect = 1, []
    for d in reversed(tail):
        expect.insert(0, want)
        want *= d
    assert all(d == 1 or s == e for d, s, e in zip(tail, x.stride()[-inner:], expect)), f"SpatialQNet: the last {inner} dimensions of {what} must be contiguous"
    if per_agent:
        assert x.shape[2] == agents, f"SpatialQNet: {what} has {x.shape[2]} agent views, agents = {agents}"
        return x.stride(0), x.stride(2), x.stride(1)
    return x.stride(0), 0, x.stride(1)


class SpatialFeed:
    """Raw rows to kernel inputs for ``n`` windows of ``T`` states: the reused ``_make_obs`` buffers of ``n * T`` rows, ONE ``susnet_featurize``
    launch per ``featurize``, and the tensors ``susnet_spatial_forward`` / ``susnet_spatial_train_step`` read where they lie -- ``spatial``
    (the Perspective featurizer's per-agent views ``[n, T, A, C, N, N]``, the Global featurizer's shared planes ``[n, T, C, N, N]``) and
    ``non_spatial`` ``[n, T, A, Fn]`` (the Global rows with every agent's one-hot appended, model_ready.py:291-306: the one-hot columns are
    written once, here; ``finish`` copies the rest behind a launch).  The actor keeps one, the trainer two (states and next states)."""

    def __init__(self, env, featurizer, n: int, T: int):
        from .features import GlobalFeaturizer

        self.env, self.n, self.T = env, n, T
        self.spec, planes, self._non = env._make_obs(featurizer.config, 1, rows=n * T)
        self.spatial, self._glob = planes.view(n, T, *planes.shape[1:]), None
        if isinstance(featurizer, GlobalFeaturizer):
            A = env.n_agents
            Fn = self._non.shape[-1] + A
            self._glob = torch.empty(n, T, A, Fn, dtype=torch.float32, device=env.device)
            self._glob[..., Fn - A:] = torch.eye(A, dtype=torch.float32, device=env.device)
        self.non_spatial = self._glob if self._glob is not None else self._non.view(n, T, *self._non.shape[1:])

    def featurize(self, rows: torch.Tensor) -> None:
        """The launch (on the caller's device context; the featurizer's row check is the caller's to poll)."""
        env = self.env
        L.check(env.lib.susnet_featurize(env._h, rows.data_ptr(), env._ROW_DTYPES[rows.dtype], self.n * self.T, C.byref(self.spec), env._stream()))

    def finish(self) -> None:
        """Behind ``featurize``: the Global featurizer's non-spatial columns into the per-agent rows (nothing to do for Perspective)."""
        if self._glob is not None:
            base = self._non.shape[-1]
            self._glob[..., :base] = self._non.view(self.n, self.T, 1, base)

    def strides(self, agents: int):
        """``(spatial, non_spatial)`` strides, three each, as the io structs take them."""
        return spatial_strides(self.spatial, 3, agents, "spatial"), spatial_strides(self.non_spatial, 1, agents, "non_spatial")


class SpatialQNet:
    """A reference ``SpatialDQN`` served by ``susnet_spatial_forward``: the module's EVAL-mode forward (dqn.py:205-301) as two HIP kernels on
    the featurizers' ``(spatial, non_spatial)`` tensors where they lie.  ``SpatialQNet(env, model)`` is None for anything the kernels do not
    serve (``spatial_desc``) -- another module, a non-square kernel / stride / padding / dilation, kernel sizes other than 1, 3, 5, an RNN that
    is not a unidirectional tanh ``nn.RNN`` with biases, a per-channel PReLU, a bound of ``include/susnet.h`` exceeded (callers then run the module).

    Like ``DenseQNet`` nothing is packed or cached: every ``forward`` takes the parameters' ``data_ptr()``s afresh, so ``optimizer.step`` and
    ``load_state_dict`` are followed without a refresh.  The RNN-input workspace ``[n, T, R]`` and the default output buffer are owned and
    re-made when the shape changes.

    ``SpatialQNet(env, model, act_dropout_seed=s)`` (opt-in) also serves the module's TRAINING-mode forward: ``forward`` then follows
    ``model.training`` as torch does -- nn.RNN's dropout between the layers through ``susnet_spatial_forward_dropout`` under the library's
    masks of seed ``s``, or the eval-mode call -- which is how the reference's never-``eval()``ed models act (train.py:104, 355-381)."""

    def __new__(cls, env, model, act_dropout_seed: Optional[int] = None):
        desc = spatial_desc(model)
        if desc is None:
            return None
        self = super().__new__(cls)
        self.env, self.model, self.desc = env, model, desc
        self.N, self.C, self.Fn, self.R, self.k, self.dims = (desc[f] for f in ("N", "C", "Fn", "R", "k", "dims"))
        self._q = self._rnn_in = None
        self.act_dropout_seed = None if act_dropout_seed is None else int(act_dropout_seed) & (2**64 - 1)
        return self

    def act_dropout_p(self) -> float:
        """The dropout probability the next ``forward`` acts under, following the module's mode as torch does: ``rnn.dropout`` for a
        training-mode model with several RNN layers on an object built with ``act_dropout_seed``, else 0 (``model.eval()``, one layer,
        ``rnn_dropout = 0``, no seed: the eval-mode forward)."""
        rnn = self.desc["rnn"]
        if self.act_dropout_seed is None or not self.model.training or rnn.num_layers < 2:
            return 0.0
        return float(rnn.dropout)

    @torch.no_grad()
    def forward(self, spatial: torch.Tensor, non_spatial: torch.Tensor, agents: int = 1, out: Optional[torch.Tensor] = None,
                net: int = 2, offset: int = 0, row_base: int = 0) -> torch.Tensor:
        """Q rows ``[B * agents, n_actions]`` (row ``b * agents + i`` = env b, agent i) of the featurizers' tensors as they are:
        ``spatial`` ``[B, T, A, C, N, N]`` (PerspectiveFeaturizer) or ``[B, T, C, N, N]`` (GlobalFeaturizer's shared planes: every agent
        reads the same image), ``non_spatial`` ``[B, T, A, Fn]`` or ``[B, T, Fn]``.  ``out``: where they go (default: a buffer this object
        keeps: a result is valid until the next call).  Two launches, asynchronous.

        Built with ``act_dropout_seed`` the call follows the module's mode (``act_dropout_p``): a training-mode model with
        ``rnn_dropout > 0`` between several layers acts under nn.RNN's inter-layer dropout (``susnet_spatial_forward_dropout``), its mask
        that of ``net`` (2: the imposters' acting network, 3: the crew's), the acting tick ``offset`` and the envs
        ``row_base .. row_base + B - 1`` (include/susnet.h); otherwise the three are not looked at.  Without a seed such a model is refused,
        as it always was."""
        env, model, desc, rnn = self.env, self.model, self.desc, self.desc["rnn"]
        if self.act_dropout_seed is None and model.training and rnn.dropout > 0 and rnn.num_layers > 1:
            raise RuntimeError("SpatialQNet: the model is in training mode with rnn_dropout > 0 between its RNN layers; the kernels compute the "
                               "eval-mode forward (no dropout): call model.eval(), or run the torch module")
        p = self.act_dropout_p()
        dev = env.device
        assert spatial.device == dev and non_spatial.device == dev, f"SpatialQNet: inputs on {dev}"
        agents = int(agents)
        sp = spatial_strides(spatial, 3, agents, "spatial")
        ns = spatial_strides(non_spatial, 1, agents, "non_spatial")
        B, T = spatial.shape[:2]
        assert tuple(spatial.shape[-3:]) == (self.C, self.N, self.N) and non_spatial.shape[-1] == self.Fn and tuple(non_spatial.shape[:2]) == (B, T), (
            f"SpatialQNet: spatial [.., {self.C}, {self.N}, {self.N}] and non_spatial [.., {self.Fn}] with the same [B, T], got "
            f"{tuple(spatial.shape)} and {tuple(non_spatial.shape)}")
        n = B * agents
        out = _out_rows(self, out, n, dev)
        if self._rnn_in is None or tuple(self._rnn_in.shape) != (n, T, self.R):
            self._rnn_in = torch.empty(n, T, self.R, dtype=torch.float32, device=dev)
        ptr = partial(_param_ptr, dev, "SpatialQNet")
        io = L.SpatialIO()
        fill_spatial_net(io, desc, T)
        for l, m in enumerate(desc["conv_modules"]):
            io.conv_weight[l], io.conv_bias[l] = ptr(m.weight), ptr(m.bias)
        for l in range(rnn.num_layers):
            for name, field in (("weight_ih", io.w_ih), ("weight_hh", io.w_hh), ("bias_ih", io.b_ih), ("bias_hh", io.b_hh)):
                field[l] = ptr(getattr(rnn, f"{name}_l{l}"))
        fill_stack(io, desc["linears"], desc["acts"], ptr)
        io.spatial, io.non_spatial = spatial.data_ptr(), non_spatial.data_ptr()
        for d in range(3):
            io.spatial_stride[d], io.non_spatial_stride[d] = sp[d], ns[d]
        io.agents, io.n, io.rnn_in, io.q_out = agents, n, self._rnn_in.data_ptr(), out.data_ptr()
        with env._on_device():
            if p > 0.0:
                drop = L.RnnDropout()
                drop.p[int(net) - 2 if int(net) in (2, 3) else 0] = p  # (a net outside 2 .. 3 is the library's to refuse)
                drop.seed, drop.offset, drop.row_base = self.act_dropout_seed, int(offset), int(row_base)
                L.check(env.lib.susnet_spatial_forward_dropout(env._h, C.byref(io), C.byref(drop), int(net), env._stream()))
            else:
                L.check(env.lib.susnet_spatial_forward(env._h, C.byref(io), env._stream()))
        return out


def _weights_version(model) -> int:
    """Changes whenever a parameter of ``model`` is written in place (optimizer.step, load_state_dict, target sync) or replaced."""
    return 0 if model is None else sum(p._version + id(p) for p in model.parameters())


def served_by_kernels(policy):
    """``(imposters served, crew served, any dense)`` of a policy object: whether each team's Q rows come from one of the library's network
    kernels (``fused_*``: the compiled-in layouts; ``dense_*``: ``susnet_mlp_forward``; ``spatial_*``: ``susnet_spatial_forward``, a
    ``WindowedPolicyRollout(kernels=True)`` -- ``acts_per_agent`` tells that kind apart) -- a crew without a model is random, which is
    served."""
    dense_imp, dense_crew = getattr(policy, "dense_imposter", None), getattr(policy, "dense_crew", None)
    if acts_per_agent(policy):
        return policy.spatial_imposter is not None, policy.crew_model is None or policy.spatial_crew is not None, False
    imp = policy.fused_imposter is not None or dense_imp is not None
    crew = policy.crew_model is None or policy.fused_crew is not None or dense_crew is not None
    return imp, crew, dense_imp is not None or dense_crew is not None


def acts_per_agent(policy) -> bool:
    """Whether ``policy`` gives one Q row per (env, agent) -- a ``WindowedPolicyRollout``: its ticks go through
    ``env.agent_policy_tick_into`` -- and not one per env (``PolicyRollout``: ``env.policy_tick_into``)."""
    return isinstance(policy, WindowedPolicyRollout)


def acting_kind(policy):
    """``(kind, imposters served, crew served)``: ``served_by_kernels`` / ``acts_per_agent`` in one answer, for ``BlockActor`` and the training run's
    checks -- ``'per_agent'``, ``'dense'`` (a ``PolicyRollout`` with a dense network: ``q_rows()``) or ``'fused'`` (the compiled-in layouts)."""
    imp, crew, dense = served_by_kernels(policy)
    return ("per_agent" if acts_per_agent(policy) else "dense" if dense else "fused"), imp, crew


def check_random_crew_stream(who: str, env, policy) -> None:
    """A crew without a model, acting through ``susnet_policy_step`` / ``susnet_agent_policy_actions``, draws from the philox stream."""
    if policy.crew_model is None and env.rng_kind != "philox":
        raise ValueError(f"{who}: a random crew draws from the production stream: build the env with rng='philox'")


def check_policy_step_actions(who: str, env, tail: str = "") -> None:
    """``susnet_policy_step``'s limit for Q rows the caller hands in (``tail``: what a caller adds to the message)."""
    if max(env.n_imposter_actions, env.n_crew_actions) > 16:
        raise ValueError(f"{who}: susnet_policy_step takes at most 16 actions per team, this game has {env.n_imposter_actions} / "
                         f"{env.n_crew_actions}{tail}")


class BlockActor:
    """THE acting loop of ``DeviceReplayBuffer.collect`` and ``evaluate``: fills slots ``0 .. n - 1`` of a feed (``env.alloc_feed``) with
    policy ticks, block after block.  Built once per sequence of blocks; ``form`` is decided here, once:

    * ``'block'``: the whole block in ONE launch (``env.policy_rollout_into``: ``susnet_qnet_policy_rollout``) -- a fused policy on an env
      that serves the whole tick in one kernel (``one_kernel``), ``one_launch_per_block``, and the block's observation slots 16-byte
      aligned (``n_block == 1 or (B * state_size) % 16 == 0``);
    * ``'ticks'``: every other fused policy, tick by tick (``env.policy_tick_into(net_imposter=...)``: one kernel where ``one_kernel``, else
      the network launch(es) + ``susnet_policy_step``; ``evaluate`` refuses the latter, ``collect`` takes it);
    * ``'dense'``: per tick ``env.refresh_obs()`` (``policy_tick_into`` writes the raw state into the feed, not ``env.obs``), at T > 1
      ``policy.push`` with the PREVIOUS slot's flags, ``policy.q_rows()``, then the ``'ticks'`` form's call with Q rows for networks;
    * ``'per_agent'``: per tick ``policy.push`` from the previous slot (flags and state), ``policy.q_rows()`` (one row per (env, agent)),
      ``env.agent_policy_tick_into``.

    ``last`` is the previous slot of this sequence (None before its first tick) and carries over block boundaries: one feed per sequence.
    ``refresh_obs_after``: the caller ends with ``env.refresh_obs()`` (dense, per-agent).  Nothing is refused here: the callers refuse."""

    def __init__(self, env, policy, epsilon: float, mask_dead: bool, n_block: int, one_launch_per_block: bool = True):
        self.env, self.policy, self.epsilon, self.mask_dead, self.n_block = env, policy, epsilon, mask_dead, n_block
        self.kind, self.imp_served, self.crew_served = acting_kind(policy)
        self.windowed = self.kind != "per_agent" and getattr(policy, "sequence_length", 1) > 1
        aligned = n_block == 1 or (env.batch * env.flattened_state_size) % 16 == 0
        self.form = self.kind if self.kind != "fused" else "block" if one_launch_per_block and self.one_kernel and aligned else "ticks"
        self.refresh_obs_after = self.kind != "fused"
        self.start()

    @cached_property
    def one_kernel(self) -> bool:
        """Whether the env serves this fused, served policy's whole tick in one kernel: asked of the env on first use, not before."""
        return (self.kind == "fused" and self.imp_served and self.crew_served and
                self.env.supports_qnet_policy_step(self.policy.fused_imposter, self.policy.fused_crew, self.epsilon))

    def start(self, fill_window: bool = False) -> None:
        """A new sequence of blocks.  ``fill_window``: the caller has not loaded the policy's window, it becomes the env's current state T
        times (train.py:318-322) -- per agent here and now, dense at the first tick behind its ``refresh_obs`` (no extra launch)."""
        self.last, self.fill_window = None, fill_window
        if fill_window and self.form == "per_agent":
            self.policy.reset_window()

    def fill(self, feed, n: int) -> None:
        """Slots ``0 .. n - 1`` of ``feed``, ``n <= n_block``: one block."""
        env, policy, epsilon, mask_dead, last = self.env, self.policy, self.epsilon, self.mask_dead, self.last
        if self.form == "block":
            env.policy_rollout_into(feed, n, policy.fused_imposter, epsilon=epsilon, mask_dead=mask_dead, net_crew=policy.fused_crew)
        elif self.form == "per_agent":
            for t in range(n):
                if last is not None:
                    policy.push(feed["done"][last], feed["truncated"][last], feed["obs"][last])
                q_imp, q_crew = policy.q_rows()
                env.agent_policy_tick_into(feed, t, q_imp, q_crew, epsilon=epsilon, mask_dead=mask_dead)
                last = t
        else:  # 'ticks' / 'dense': env.policy_tick_into by the packed networks, or by the Q rows of the tick's q_rows()
            dense, windowed, fill_window = self.form == "dense", self.windowed, self.fill_window
            net_imp, net_crew = (None, None) if dense else (policy.fused_imposter, policy.fused_crew)
            q_imp = q_crew = None
            for t in range(n):
                if dense:
                    env.refresh_obs()
                    if windowed and last is not None:
                        policy.push(feed["done"][last], feed["truncated"][last])
                    elif windowed and fill_window:  # the first tick of the sequence only: `last` is a slot from here on
                        policy.reset_window()
                    q_imp, q_crew = policy.q_rows()
                env.policy_tick_into(feed, t, net_imposter=net_imp, net_crew=net_crew, q_imposter=q_imp, q_crew=q_crew, epsilon=epsilon, mask_dead=mask_dead)
                last = t  # (read by the dense form's push alone)
        self.last = last


class PolicyRollout:
    """Greedy policy-in-the-loop stepping of a batched env.

    Per tick: the flat observation (written by the previous step / reset kernel) feeds ``imposter_model`` and
    ``crew_model``; agent *i* of env *b* takes the imposter model's argmax if it is an imposter there, else the
    crew model's (all agents see the same flat features, as in the reference's FlatFeaturizer,
    model_ready.py:356-367).  ``crew_model=None`` = uniformly random crew via the env's sample_actions kernel.

    ``sequence_length=T`` > 1 (with ``dense=True``): the networks read the WINDOW of the last T states' feature rows, oldest first
    (train.py:318-322, 388-389, 441-445; dqn.py:86-90), so their input width is ``T * F``.  The policy owns two ``[B, T * F]`` buffers;
    ``window_feats`` is the current one, ``q_rows()`` feeds it to the dense kernel, ``push(done, truncated)`` moves it one tick on
    (``susnet_window_push`` with ``fresh = env.obs``, out of place: the buffers swap), ``tick()`` pushes with the flags the step
    returned, ``reset_window()`` refills it with the current state (after ``env.reset()``).  Only dense-served networks are accepted at
    T > 1 (``WindowedPolicyRollout`` is the torch path for everything else).
    """

    def __init__(self, env, imposter_model: nn.Module, crew_model: Optional[nn.Module] = None,
                 components: Sequence[str] = ("onehot_pos",), fused: bool = True, epsilon: float = 0.0, mask_dead: bool = False,
                 dense: bool = False, sequence_length: int = 1):
        assert env.obs_config.mode == "flat" and list(env.obs_config.components) == list(components), (
            "construct the env with obs=ObsConfig('flat', components) so that step() fuses the observation")
        self.env, self.imposter_model, self.crew_model = env, imposter_model, crew_model
        # epsilon-greedy acting as in the trainer (train.py:355-381; `epsilon` may be changed between ticks: the scheduler's value) and its
        # habit of giving dead agents index 0; both are applied by the kernels that choose the actions (PHILOX handles)
        self.epsilon, self.mask_dead = float(epsilon), bool(mask_dead)
        # reference MLPs on a compiled-in feature layout run as ONE kernel from the state words to the Q row (susnet_qnet_forward);
        # with `dense=True` every other reference MLP within the dense kernel's widths -- any game, component set, layer stack -- runs
        # as one kernel on env.obs (susnet_mlp_forward: dense_imposter / dense_crew): what collect / train / evaluate need on those
        # games.  It is OFF by default: measured at 65 536 rows the kernel takes 2.2 - 3.3 x the torch modules' time
        # (profiles/dense_qnet_bench.json), so plain acting keeps the torch module on env.obs, as does anything else (SpatialDQN, wider
        # stacks)
        self.components = list(components)
        T = self.sequence_length = int(sequence_length)
        if T < 1:
            raise ValueError(f"PolicyRollout: sequence_length = {sequence_length} (a window holds at least one state)")
        if T > 1:  # the compiled-in layouts read ONE state's F features: they never serve a window
            fused_nets = False
        else:
            fused_nets = fused
        self.fused_imposter = pack_mlp(env, imposter_model, components) if fused_nets else None
        self.fused_crew = pack_mlp(env, crew_model, components) if fused_nets and crew_model is not None else None
        self.dense_imposter = self._dense(imposter_model, env.n_imposter_actions) if fused and dense and self.fused_imposter is None else None
        self.dense_crew = self._dense(crew_model, env.n_crew_actions) if fused and dense and crew_model is not None and self.fused_crew is None else None
        self._packed_version = (_weights_version(imposter_model), _weights_version(crew_model))
        # ... and with a random crew on one of the compiled-in games the whole tick -- network, argmax, the crew's draws, the step -- is
        # ONE kernel (susnet_qnet_policy_step); so it is with both teams' networks (round 5: the LDS image is swapped between the two passes)
        self.one_kernel_tick = (self.fused_imposter is not None and (crew_model is None or self.fused_crew is not None) and
                                env.supports_qnet_policy_step(self.fused_imposter, self.fused_crew, self.epsilon))
        B = env.batch
        self._spatial = torch.zeros(B, 1, 1, device=env.device)  # FlatFeaturizer's dummy spatial input
        self._actions = torch.zeros(B, env.n_agents, dtype=torch.int64, device=env.device)
        self._windows, self._window_at, self._window_generation = None, 0, None
        if T > 1:
            self._check_window_served(fused and dense)
            F = env.obs.shape[-1]
            self._windows = [torch.zeros(B, T * F, dtype=torch.float32, device=env.device) for _ in range(2)]  # ping / pong

    def _dense(self, model, n_actions):
        net = DenseQNet(self.env, model)
        if net is None or net.dims[0] != self.sequence_length * self.env.obs.shape[-1] or net.dims[-1] != n_actions:
            return None
        return net

    def _check_window_served(self, asked: bool) -> None:
        """At ``sequence_length`` > 1 there is no torch path in this class: a network the dense kernel does not serve is an error."""
        env, T = self.env, self.sequence_length
        F = env.obs.shape[-1]
        need = (f"PolicyRollout: sequence_length = {T} is served through the dense kernel only (dense=True): reference MLPs whose input is the "
                f"flattened window, T * F = {T} * {F} = {T * F} <= {L.MLP_MAX_F} wide, on a game with at most 16 actions per team "
                "(WindowedPolicyRollout runs everything else through torch)")
        if not asked:
            raise ValueError(need + "; got dense=False")
        if T > L.WINDOW_MAX_T or T * F > L.MLP_MAX_F:
            raise ValueError(need + f"; this window is {T} states, {T * F} features wide")
        if max(env.n_imposter_actions, env.n_crew_actions) > 16:
            raise ValueError(need + f"; this game has {env.n_imposter_actions} / {env.n_crew_actions} actions")
        for team, model, net in (("imposter", self.imposter_model, self.dense_imposter), ("crew", self.crew_model, self.dense_crew)):
            if model is not None and net is None:
                stack = _mlp_stack(model)
                got = f"an MLP with {stack[0][0].in_features} inputs" if stack is not None else type(model).__name__
                raise ValueError(need + f"; the {team} model is {got}")

    @property
    def window_feats(self) -> Optional[torch.Tensor]:
        """The current feature window ``[B, T * F]`` (oldest state first), or None at ``sequence_length`` 1."""
        return None if self._windows is None else self._windows[self._window_at]

    @torch.no_grad()
    def reset_window(self) -> torch.Tensor:
        """``window_feats`` = ``env.obs`` repeated T times (train.py:318-322): the window of a fresh episode, or of the current state."""
        assert self._windows is not None, "reset_window: built with sequence_length = 1, there is no window"
        env = self.env
        self._windows[self._window_at].copy_(env.obs.repeat(1, self.sequence_length))
        self._window_generation = getattr(env, "reset_generation", 0)
        return self.window_feats

    def load_window(self) -> torch.Tensor:
        """The current buffer, for a caller that is about to WRITE the window itself (``DeviceReplayBuffer.collect`` featurizes its
        carried raw window into it): marks the window as belonging to the env's current episode generation."""
        assert self._windows is not None, "load_window: built with sequence_length = 1, there is no window"
        self._window_generation = getattr(self.env, "reset_generation", 0)
        return self.window_feats

    def _window_current(self) -> None:
        if self._window_generation != getattr(self.env, "reset_generation", 0):  # never filled, or the env was reset() since
            self.reset_window()

    @torch.no_grad()
    def push(self, done: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The window one tick on (``susnet_window_push``, one launch, asynchronous): ``env.obs`` -- the state AFTER the tick -- enters as the
        newest state, or fills the window where ``done | truncated`` (bool / uint8 ``[B]`` on the env's device, read in place; None: no row
        ended).  The two buffers swap; returns the new ``window_feats``."""
        assert self._windows is not None, "push: built with sequence_length = 1, there is no window"
        env = self.env
        self._window_current()
        src, dst = self._windows[self._window_at], self._windows[self._window_at ^ 1]
        io = L.WindowIO()
        io.fresh, io.src, io.dst = env.obs.data_ptr(), src.data_ptr(), dst.data_ptr()
        for name, flag in (("done", done), ("truncated", truncated)):
            if flag is not None:
                assert flag.dtype in (torch.bool, torch.uint8) and flag.numel() == env.batch and flag.is_contiguous() and flag.device == env.device, (
                    f"push: {name} must be a contiguous bool / uint8 [{env.batch}] tensor on {env.device}")
                setattr(io, name, flag.data_ptr())
        io.T, io.F, io.n = self.sequence_length, env.obs.shape[-1], env.batch
        with env._on_device():
            L.check(env.lib.susnet_window_push(env._h, C.byref(io), env._stream()))
        self._window_at ^= 1
        return dst

    def _team_q(self, fused, dense, model, feats):
        if fused is not None:
            return self.env.qnet_forward(fused)
        if dense is not None:
            return dense.forward(feats)
        return model(self._spatial, feats)

    def refresh_weights(self, force: bool = True) -> bool:
        """Re-pack the models' CURRENT weights into the device images the fused kernels read (in place: a captured graph keeps
        reading the same buffers).  The acting loop of the trainer changes the weights between ticks (optimizer.step, target sync:
        train.py:402-416); ``tick()`` / ``act()`` / ``q_rows()`` call this with ``force=False`` -- a version check of the parameters --
        so eager loops follow the modules by themselves, but a REPLAYED graph runs no host code: call ``refresh_weights()`` before
        ``graph.replay()`` after changing weights.  Returns whether anything was re-packed."""
        ver = (_weights_version(self.imposter_model), _weights_version(self.crew_model))
        if not force and ver == self._packed_version:
            return False
        if self.fused_imposter is not None:
            pack_mlp(self.env, self.imposter_model, self.components, into=self.fused_imposter)
        if self.fused_crew is not None:
            pack_mlp(self.env, self.crew_model, self.components, into=self.fused_crew)
        self._packed_version = ver
        return self.fused_imposter is not None or self.fused_crew is not None

    def state_dict(self) -> dict:
        """What a ``PolicyRollout`` keeps between two ``collect`` calls that nothing else holds: nothing.  The weights are
        the modules' (the trainer saves them), the packed images are re-packed from them, and the feature window is derived from the
        ring's carried raw window at the start of every ``collect``."""
        return {"kind": "PolicyRollout", "sequence_length": self.sequence_length}

    def load_state_dict(self, sd: dict) -> None:
        """After the models' weights were restored: a forced ``refresh_weights``, so that the fused images are re-packed from them, and a
        feature window that belongs to no episode generation (the next ``collect`` / ``q_rows`` fills it)."""
        if sd.get("kind") != "PolicyRollout" or int(sd["sequence_length"]) != self.sequence_length:
            raise ValueError(f"load_state_dict: saved from a {sd.get('kind')} with sequence_length = {sd.get('sequence_length')}, this is a "
                             f"PolicyRollout with sequence_length = {self.sequence_length}")
        self._window_generation = None
        self.refresh_weights(force=True)

    @torch.no_grad()
    def q_rows(self):
        """The teams' Q rows on the current observation: ``(q_imposter [B, n_imposter_actions], q_crew or None)``."""
        env = self.env
        self.refresh_weights(force=False)
        feats = env.obs  # [B, F] float32, refreshed by reset()/step()
        if self._windows is not None:  # [B, T * F]: the last T states' rows, oldest first
            self._window_current()
            feats = self.window_feats
        q_imp = self._team_q(self.fused_imposter, self.dense_imposter, self.imposter_model, feats)
        q_crew = None
        if self.crew_model is not None:
            q_crew = self._team_q(self.fused_crew, self.dense_crew, self.crew_model, feats)
        return q_imp.contiguous(), (q_crew.contiguous() if q_crew is not None else None)

    @torch.no_grad()
    def tick(self):
        """One tick of the acting loop (visualize.py:547-582): Q rows, greedy actions, env.step.  Returns ``(actions, rewards, done,
        truncated)``.  ONE launch where the env serves it (``susnet_qnet_policy_step``: a reference MLP for the imposters, a random crew, a
        compiled-in game); else two (the network, then ``susnet_policy_step``: argmax, the crew's draws and the step in one kernel); else
        ``act()`` + ``env.step``."""
        env = self.env
        if self.one_kernel_tick:
            self.refresh_weights(force=False)
            _, rew, done, trunc, _, a = env.qnet_policy_step(self.fused_imposter, actions_out=self._actions, epsilon=self.epsilon, mask_dead=self.mask_dead,
                                                             net_crew=self.fused_crew)
            return a, rew, done, trunc
        q_imp, q_crew = self.q_rows()
        fits = max(env.n_imposter_actions, env.n_crew_actions) <= 16 and (q_crew is not None or env.rng_kind == "philox")
        if fits:
            _, rew, done, trunc, _, a = env.policy_step(q_imp, q_crew, actions_out=self._actions, epsilon=self.epsilon, mask_dead=self.mask_dead)
        else:
            a = self.act()
            _, rew, done, trunc, _ = env.step(a)
        if self._windows is not None:  # (the step has written the new state's row into env.obs)
            self.push(done, trunc)
        return a, rew, done, trunc

    @torch.no_grad()
    def act(self) -> torch.Tensor:
        """One tick's actions: the network forward(s) through stock PyTorch-ROCm, then ONE kernel (``susnet_policy_actions``) that
        reads the episode's roles from the env's state, takes each team's argmax and -- without a crew network -- the crew's
        draws from the action stream.  (The eager form of the same thing -- role export, argmax, sample_actions, dtype copy,
        where -- was five launches and a tenth of the tick's GPU time.)"""
        env = self.env
        q_imp, q_crew = self.q_rows()
        if env.rng_kind != "philox" and q_crew is None:  # numpy tapes: the crew's draws come from the env's own words (greedy only)
            assert not self.epsilon and not self.mask_dead, "epsilon-greedy / mask_dead act through the production stream: rng='philox'"
            if not env.export_state:
                env.refresh_roles()
            torch.where(env.imposter_mask, q_imp.argmax(dim=1).unsqueeze(1), env.sample_actions().to(torch.int64), out=self._actions)
            return self._actions
        return env.policy_actions(q_imp, q_crew, out=self._actions, epsilon=self.epsilon, mask_dead=self.mask_dead)

    @torch.no_grad()
    def run(self, n_steps: int, record: bool = False, block_ticks: int = 64) -> Dict[str, torch.Tensor]:
        """``n_steps`` ticks of the acting loop with the networks as they are (``run_game``, visualize.py:547-582).  Where the env serves the
        whole tick as one kernel and nothing is recorded, ``block_ticks`` ticks go into ONE launch (``susnet_qnet_policy_rollout``; 0: one
        launch per tick)."""
        env = self.env
        if self.one_kernel_tick and not record and block_ticks > 0 and env.auto_reset:
            self.refresh_weights(force=False)
            left = int(n_steps)
            while left > 0:
                n = min(left, int(block_ticks))
                env.policy_block(n, self.fused_imposter, epsilon=self.epsilon, mask_dead=self.mask_dead, net_crew=self.fused_crew)
                left -= n
            return {}
        out: Dict[str, List[torch.Tensor]] = {"actions": [], "rewards": [], "done": [], "truncated": []}
        for _ in range(n_steps):
            a, rew, done, trunc = self.tick()
            if record:
                out["actions"].append(a.clone())
                out["rewards"].append(rew.clone())
                out["done"].append(done.clone())
                out["truncated"].append(trunc.clone())
        return {k: torch.stack(v) for k, v in out.items()} if record else {}


    @torch.no_grad()
    def capture(self, n_ticks: int = 8, record: bool = False):
        """The policy tick -- {roles refresh, network forward, argmax, crew sampling, where, env step} x ``n_ticks`` -- as ONE
        hipGraph (reference loop shape: visualize.py:547-582, one Python iteration per tick).  Everything a tick touches is
        device-resident (the env's step counter included: ``device_tick``), so ``graph.replay()`` advances the rollout by
        ``n_ticks`` ticks with a single launch from the host instead of ~20 eager launches per tick.

        Returns ``(graph, outputs)``; with ``record=True`` ``outputs`` holds static ``actions / rewards / done / truncated /
        obs_before`` tensors with a leading ``[n_ticks]`` dimension that every replay overwrites (parity tests).  Needs an env
        built with ``rng='philox', check_errors=False, export_state=False`` (both would synchronise inside the capture)."""
        env = self.env
        if self._windows is not None:
            raise ValueError(f"capture: sequence_length = {self.sequence_length}: the window's two buffers swap every tick, a captured graph would "
                             "freeze their pointers; graph capture serves sequence_length = 1")
        assert env.rng_kind == "philox", "graph replay needs the counter-based production stream"
        assert not env.check_errors and not env.export_state, "construct the env with check_errors=False, export_state=False"
        env.device_tick(True)
        B, A = env.batch, env.n_agents
        out: Dict[str, torch.Tensor] = {}
        if record:
            out = {"actions": torch.zeros(n_ticks, B, A, dtype=torch.int64, device=env.device),
                   "rewards": torch.zeros(n_ticks, B, A, dtype=torch.float32, device=env.device),
                   "done": torch.zeros(n_ticks, B, dtype=torch.bool, device=env.device),
                   "truncated": torch.zeros(n_ticks, B, dtype=torch.bool, device=env.device),
                   "obs_before": torch.zeros(n_ticks, *env.obs.shape, dtype=env.obs.dtype, device=env.device)}

        def tick(k):
            if record:
                out["obs_before"][k].copy_(env.obs)
            a, rew, done, trunc = self.tick()
            if record:
                out["actions"][k].copy_(a)
                out["rewards"][k].copy_(rew)
                out["done"][k].copy_(done)
                out["truncated"][k].copy_(trunc)

        cur = torch.cuda.current_stream(env.device)
        side = torch.cuda.Stream(env.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # warm-up on a side stream, as torch's capture rules ask (these ticks count: the rollout advances)
            for k in range(2):
                tick(k % n_ticks)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for k in range(n_ticks):
                tick(k)
        self.captured_warmup_ticks = 2
        return graph, out


class WindowedPolicyRollout:
    """Acting loop over a device-resident window of the last ``sequence_length`` flattened states per env.

    ``env`` must fuse the raw uint8 observation into step/reset (``obs=ObsConfig('raw', dtype=torch.uint8)``) and
    auto-reset.  ``featurizer`` is one of ``features.PerspectiveFeaturizer / GlobalFeaturizer / FlatFeaturizer`` built on
    the same env.  Per tick (train.py:345-383): ``featurizer.fit(window)``; agent *i* of env *b* acts by the imposter
    network if it is an imposter there, else by the crew network, on ITS view; dead agents get index 0 when
    ``mask_dead`` (train.py) and act like everybody else otherwise (visualize.py:547-560); with ``epsilon`` > 0 a
    uniformly random role-valid index replaces the greedy one with that probability (the env's sample_actions kernel
    supplies it).
    """

    def __init__(self, env, featurizer, imposter_model: nn.Module, crew_model: Optional[nn.Module], sequence_length: int = 2,
                 epsilon: float = 0.0, mask_dead: bool = True, seed: int = 0, kernels: bool = False, act_dropout_seed: Optional[int] = None):
        assert env.obs_config.mode == "raw" and env.obs_config.dtype == torch.uint8 and env.auto_reset, (
            "construct the env with obs=ObsConfig('raw', dtype=torch.uint8), auto_reset=True")
        self.env, self.featurizer = env, featurizer
        self.imposter_model, self.crew_model = imposter_model, crew_model
        self.T, self.epsilon, self.mask_dead = int(sequence_length), float(epsilon), mask_dead
        # kernels=True: a team whose model SpatialQNet serves gets its Q rows for all B * A (env, agent) rows from ONE susnet_spatial_forward
        # per tick, on the featurizer's buffers in place; a model that is not served keeps the torch modules below, per team.  Off by default
        # act_dropout_seed (with kernels=True): the SpatialQNets are built with it, so a team whose model is in training mode acts under
        # nn.RNN's dropout between its layers, as the reference's agents do (train.py never calls eval()): net 2 the imposters', net 3 the
        # crew's.  act_ticks is the mask offset of the NEXT q_rows() / act(): it advances by one per call that ran a team under dropout
        self.act_dropout_seed = None if act_dropout_seed is None else int(act_dropout_seed) & (2**64 - 1)
        self.act_ticks = 0
        self.spatial_imposter = self._spatial(imposter_model, env.n_imposter_actions) if kernels else None
        self.spatial_crew = self._spatial(crew_model, env.n_crew_actions) if kernels else None
        self._gen = torch.Generator(device=env.device)
        self._gen.manual_seed(seed)
        self.window = None
        self._actions = torch.zeros(env.batch, env.n_agents, dtype=torch.int64, device=env.device)
        self._feed = None  # q_rows(): the SpatialFeed of the B windows

    @property
    def sequence_length(self) -> int:
        return self.T

    def _spatial(self, model, n_actions):
        from .features import GlobalFeaturizer, PerspectiveFeaturizer

        net = SpatialQNet(self.env, model, act_dropout_seed=self.act_dropout_seed)
        if net is None or not isinstance(self.featurizer, (GlobalFeaturizer, PerspectiveFeaturizer)) or self.T > L.SPATIAL_MAX_T:
            return None
        return net if spatial_feed_mismatch(self.env, self.featurizer, net.desc, n_actions) is None else None

    def kernel_inputs(self):
        """``(spatial, non_spatial)`` of the fitted featurizer as ``SpatialQNet.forward`` takes them: the Perspective featurizer's buffers in
        place; the Global featurizer's shared planes, and its non-spatial row with every agent's one-hot appended
        (``GlobalFeaturizer.generate_featurized_states``, model_ready.py:291-306) as ``[B, T, A, Fn]``."""
        from .features import GlobalFeaturizer

        f = self.featurizer
        if not isinstance(f, GlobalFeaturizer):
            return f.spatial, f.non_spatial
        A = self.env.n_agents
        B, T = f.non_spatial.shape[:2]
        eye = torch.eye(A, dtype=torch.float32, device=f.non_spatial.device)
        return f.spatial, torch.cat([f.non_spatial.unsqueeze(2).expand(B, T, A, -1), eye.expand(B, T, A, A)], dim=3)

    def reset(self):
        self.env.reset()
        self.window = self.env.obs.unsqueeze(1).repeat(1, self.T, 1)  # train.py:318-322: the first state T times
        return self.window

    # ---- the collection loop's side (DeviceReplayBuffer.collect, evaluate): the window moved in place by the library, Q rows per agent ----
    def reset_window(self) -> torch.Tensor:
        """The acting window of the env's CURRENT state: that state T times (train.py:318-322)."""
        from .env import ObsConfig

        first = self.env.observe(ObsConfig("raw", dtype=torch.uint8))
        self.window = first.unsqueeze(1).repeat(1, self.T, 1).contiguous()
        return self.window

    def load_window(self, raw_window: torch.Tensor) -> torch.Tensor:
        """The acting window := a copy of ``raw_window`` (``[B, T, S]`` uint8: e.g. the window a ring carries between ``collect`` calls)."""
        B, T, S = self.env.batch, self.T, self.env.flattened_state_size
        assert raw_window.dtype == torch.uint8 and tuple(raw_window.shape) == (B, T, S), f"load_window: uint8 [{B}, {T}, {S}]"
        if self.window is None or self.window.data_ptr() == raw_window.data_ptr() or not self.window.is_contiguous():
            self.window = torch.empty(B, T, S, dtype=torch.uint8, device=self.env.device)
        self.window.copy_(raw_window)
        return self.window

    def push(self, done: torch.Tensor, truncated: torch.Tensor, obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The acting window one tick on, in place (``susnet_state_window_push``; train.py:388-389, 441-445): ``obs`` ``[B, S]`` uint8 is the
        state after the tick (default ``env.obs``), ``done`` / ``truncated`` ``[B]`` its flags -- e.g. a feed slot, read where the stepping
        kernel wrote it.  Asynchronous."""
        env = self.env
        obs = env.obs if obs is None else obs
        B, S = env.batch, env.flattened_state_size
        assert self.window is not None and self.window.is_contiguous(), "push: no window yet (reset_window / load_window)"
        assert obs.dtype == torch.uint8 and tuple(obs.shape) == (B, S) and obs.is_contiguous(), f"push: obs is uint8 [{B}, {S}]"
        for name, f in (("done", done), ("truncated", truncated)):
            assert f.dtype in (torch.bool, torch.uint8) and tuple(f.shape) == (B,) and f.is_contiguous(), f"push: {name} is bool [{B}]"
        with env._on_device():
            L.check(env.lib.susnet_state_window_push(env._h, self.window.data_ptr(), self.T, S, B, obs.data_ptr(), done.data_ptr(),
                                                     truncated.data_ptr(), env._stream()))
        return self.window

    def refresh_weights(self, force: bool = False) -> bool:
        """Nothing to do: ``SpatialQNet`` reads the modules' parameters in place at every forward."""
        return False

    def state_dict(self) -> dict:
        """What the policy keeps between two ``collect`` calls that nothing else holds: ``act_ticks``, the mask offset of acting under
        dropout, and the state of the generator ``act()`` explores with.  The acting window is not part of it: ``collect`` loads it from
        the ring's carried raw window at the start of every call."""
        return {"kind": "WindowedPolicyRollout", "sequence_length": self.T, "act_ticks": int(self.act_ticks),
                "act_dropout_seed": self.act_dropout_seed, "generator": self._gen.get_state()}

    def load_state_dict(self, sd: dict) -> None:
        """Restore ``act_ticks`` and the exploration generator, drop the acting window (the next ``collect`` loads it) and -- for the
        interface's sake, it packs nothing -- ``refresh_weights(force=True)``.  A policy of another kind, window length or
        ``act_dropout_seed`` is a ``ValueError``."""
        mine = {"kind": "WindowedPolicyRollout", "sequence_length": self.T, "act_dropout_seed": self.act_dropout_seed}
        for k, v in mine.items():
            if sd.get(k) != v:
                raise ValueError(f"load_state_dict: the policy was saved with {k} = {sd.get(k)!r}, this one has {v!r}")
        self.act_ticks = int(sd["act_ticks"])
        self._gen.set_state(sd["generator"])
        self.window = None
        self.refresh_weights(force=True)

    @torch.no_grad()
    def q_rows(self):
        """``(q_imposter [B * A, n], q_crew [B * A, n] or None)`` of the acting window: ONE ``susnet_featurize`` launch over its ``B * T`` rows
        into reused buffers (a ``SpatialFeed``), and one ``SpatialQNet.forward`` per team that has a model.  Row ``b * A + i`` = env b, agent i; a
        result is valid until the next call.  With ``act_dropout_seed`` a team in training mode acts under dropout at offset ``act_ticks``
        (net 2 the imposters, 3 the crew), and ``act_ticks`` then advances by one; a call that is refused uses up no offset."""
        env, A = self.env, self.env.n_agents
        assert self.spatial_imposter is not None and (self.crew_model is None or self.spatial_crew is not None), (
            "q_rows: susnet_spatial_forward does not serve this policy (WindowedPolicyRollout(kernels=True) with SpatialDQN models)")
        assert self.window is not None, "q_rows: no window yet (reset_window / load_window)"
        if self._feed is None:
            self._feed = SpatialFeed(env, self.featurizer, env.batch, self.T)
        feed = self._feed
        with env._on_device():
            # (the window's rows were written by the stepping kernel: valid by construction, the featurizer's row check is not polled)
            feed.featurize(self.window)
        feed.finish()
        q_imp, q_crew = self._team_forwards(feed.spatial, feed.non_spatial)
        return q_imp, q_crew

    def _team_forwards(self, spatial, non_spatial):
        """One ``SpatialQNet.forward`` per served team on one tick's inputs (None for a team without one), imposters as net 2 and crew as
        net 3 at offset ``act_ticks``, which advances once if a team ran under dropout."""
        A, out, dropped = self.env.n_agents, [], False
        for net, qnet in ((2, self.spatial_imposter), (3, self.spatial_crew)):
            if qnet is None:
                out.append(None)
                continue
            out.append(qnet.forward(spatial, non_spatial, A, net=net, offset=self.act_ticks))
            dropped = dropped or qnet.act_dropout_p() > 0.0
        self.act_ticks += int(dropped)  # (behind both forwards: a refusal raised above has used up no offset)
        return out

    @torch.no_grad()
    def act(self) -> torch.Tensor:
        env = self.env
        if self.crew_model is None:
            raise ValueError("WindowedPolicyRollout.act: a random crew (crew_model=None) acts through q_rows() + env.agent_policy_tick_into")
        if self.window is None:
            self.reset()
        if not env.export_state:
            env.refresh_roles()
        self.featurizer.fit(self.window)
        imp_mask = env.imposter_mask  # [B, A]
        if self.spatial_imposter is None and self.spatial_crew is None:
            for i, (spatial, non_spatial) in enumerate(self.featurizer.generate_featurized_states()):
                q_imp = self.imposter_model(spatial, non_spatial).argmax(dim=1)
                q_crew = self.crew_model(spatial, non_spatial).argmax(dim=1)
                self._actions[:, i] = torch.where(imp_mask[:, i], q_imp, q_crew)
        else:
            B, A = env.batch, env.n_agents
            views = None
            if self.spatial_imposter is None or self.spatial_crew is None:
                views = self.featurizer.generate_featurized_states()
            spatial, non_spatial = self.kernel_inputs()
            greedy = []
            for q, model in zip(self._team_forwards(spatial, non_spatial), (self.imposter_model, self.crew_model)):
                if q is not None:
                    greedy.append(q.argmax(dim=1).view(B, A))
                else:
                    greedy.append(torch.stack([model(sp, ns).argmax(dim=1) for sp, ns in views], dim=1))
            torch.where(imp_mask, greedy[0], greedy[1], out=self._actions)
        if self.epsilon > 0.0:
            explore = torch.rand(self._actions.shape, device=env.device, generator=self._gen) <= self.epsilon  # train.py:359,371
            self._actions.copy_(torch.where(explore, env.sample_actions().to(torch.int64), self._actions))
        if self.mask_dead:
            self._actions.mul_(env.alive_agents.to(torch.int64) if env.export_state else self._alive_from_window())
        return self._actions

    def _alive_from_window(self) -> torch.Tensor:
        A = self.env.n_agents
        return self.window[:, -1, 2 * A:3 * A].to(torch.int64)  # flatten_state: alive flags follow the A (x, y) pairs

    @torch.no_grad()
    def step(self):
        """One tick: act, env.step, window update.  Returns (actions, rewards, done, truncated)."""
        env = self.env
        a = self.act()
        _, rew, done, trunc, _ = env.step(a)
        ended = (done | trunc).view(-1, 1, 1)
        nxt = torch.roll(self.window, shifts=-1, dims=1)  # train.py:388-389
        nxt[:, -1] = env.obs
        # an ended env was auto-reset inside the step: its window restarts from the fresh first state (train.py:452-457)
        self.window = torch.where(ended, env.obs.unsqueeze(1).expand(-1, self.T, -1), nxt)
        return a, rew, done, trunc

    @torch.no_grad()
    def run(self, n_steps: int, record: bool = False) -> Dict[str, torch.Tensor]:
        out: Dict[str, List[torch.Tensor]] = {"actions": [], "rewards": [], "done": [], "truncated": []}
        for _ in range(n_steps):
            a, rew, done, trunc = self.step()
            if record:
                for k, v in zip(out, (a, rew, done, trunc)):
                    out[k].append(v.clone())
        return {k: torch.stack(v) for k, v in out.items()} if record else {}
