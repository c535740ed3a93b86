"""CPU-only: which layer stacks each network path accepts, pinned on one table of hand-built modules.  ``policy.linear_prelu_stack`` is the
one recogniser and ``policy.stack_within_bounds`` the one statement of the dense widths; ``DenseQNet``, the trainer's two learners
(``_mlp_dims`` for the fused step, ``dense_stack`` for the dense one), ``pack_mlp`` and ``SpatialQNet``'s head are their callers.  The
expected answers are what each caller gave BEFORE it was moved onto the shared functions (recorded by running this table there), so a caller
whose accept set drifts -- or a new path that copies the conditions and gets one wrong -- fails here.  No kernel is launched."""
import ctypes as C
import importlib

import pytest
import torch
from torch import nn

BASE = [36, 256, 128, 64, 16, 6]  # the reference's architecture on the 1v1 9x9 one-hot layout: served by every path


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _edit(pkg, dims=BASE, **at):
    """``MLP(dims)`` with the layers at the given positions of its Sequential replaced (``at``: ``i3=module``)."""
    m = pkg.policy.MLP(dims)
    for k, layer in at.items():
        m.model[int(k[1:])] = layer
    return m


def _modules(pkg):
    P, F = pkg.policy, pkg._lib.MLP_MAX_F
    trailing = P.MLP(BASE)
    trailing.model = nn.Sequential(*trailing.model, nn.PReLU())
    empty = P.MLP(BASE)
    empty.model = nn.Sequential()
    return {
        "linears_1": P.MLP([36, 6]),
        "linears_5": P.MLP(BASE),
        "linears_7": P.MLP([36] + [8] * 6 + [6]),
        "linears_8": P.MLP([36] + [8] * 7 + [6]),
        "hidden_256": P.MLP([36, 256, 256, 64, 16, 6]),
        "hidden_257": P.MLP([36, 257, 128, 64, 16, 6]),
        "out_32": P.MLP(BASE[:-1] + [32]),
        "out_33": P.MLP(BASE[:-1] + [33]),
        "in_1": P.MLP([1] + BASE[1:]),
        "in_max": P.MLP([F] + BASE[1:]),
        "in_max_plus_1": P.MLP([F + 1] + BASE[1:]),
        "bias_false": _edit(pkg, i4=nn.Linear(128, 64, bias=False)),
        "prelu_per_channel": _edit(pkg, i1=nn.PReLU(256)),
        "trailing_activation": trailing,
        "relu_for_prelu": _edit(pkg, i3=nn.ReLU()),
        "unchained_width": _edit(pkg, i2=nn.Linear(200, 128)),
        "empty_sequential": empty,
        "bare_sequential": P.make_mlp(BASE),  # the right stack, but not a reference MLP module
    }


# name: (linear_prelu_stack's dims, DenseQNet's dims, the trainer's _mlp_dims, the trainer's dense dims, pack_mlp's dims); None = declined.
# Columns 2 .. 5 are the parent's answers.  Two rows show the one difference that is kept: _mlp_dims lets a trailing PReLU and unchained
# widths through (it never asked for either condition), everybody else declines them
SEVEN, WIDE = [36] + [8] * 6 + [6], [36, 256, 256, 64, 16, 6]
EXPECT = {
    "linears_1": ([36, 6], [36, 6], None, [36, 6], None),
    "linears_5": (BASE, BASE, BASE, BASE, BASE),
    "linears_7": (SEVEN, SEVEN, None, SEVEN, None),
    "linears_8": ([36] + [8] * 7 + [6], None, None, None, None),
    "hidden_256": (WIDE, WIDE, WIDE, WIDE, None),
    "hidden_257": ([36, 257, 128, 64, 16, 6], None, [36, 257, 128, 64, 16, 6], None, None),
    "out_32": (BASE[:-1] + [32], BASE[:-1] + [32], BASE[:-1] + [32], BASE[:-1] + [32], BASE[:-1] + [32]),
    "out_33": (BASE[:-1] + [33], None, BASE[:-1] + [33], None, None),
    "in_1": ([1] + BASE[1:], [1] + BASE[1:], [1] + BASE[1:], [1] + BASE[1:], None),
    "in_max": ([1024] + BASE[1:], [1024] + BASE[1:], [1024] + BASE[1:], [1024] + BASE[1:], None),
    "in_max_plus_1": ([1025] + BASE[1:], None, [1025] + BASE[1:], None, None),
    "bias_false": (None, None, None, None, None),
    "prelu_per_channel": (None, None, None, None, None),
    "trailing_activation": (None, None, BASE, None, None),
    "relu_for_prelu": (None, None, None, None, None),
    "unchained_width": (None, None, BASE, None, None),
    "empty_sequential": (None, None, None, None, None),
    "bare_sequential": (BASE, None, None, None, None),
}


class _PackEnv:
    """What ``pack_mlp`` -> ``env.qnet_pack`` reads of an env, on a handle without device buffers: the 1v1 9x9 ImposterTrainingGround, whose
    ``onehot_pos`` layout (F = 36) the fused kernels know."""

    def __init__(self, pkg):
        L = pkg._lib
        self.lib, self.device = L.lib(), torch.device("cpu")
        cfg = L.Config()
        cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
        for k, v in dict(variant=L.VARIANT_ITG, batch=8, n_imposters=1, n_crew=1, n_jobs=0, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                         shuffle_imposter_index=0, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
            setattr(cfg, k, v)
        for i in range(cfg.grid_n):
            cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
        self._h = C.c_void_p()
        assert self.lib.susnet_create(C.byref(cfg), C.byref(self._h)) == 0, self.lib.susnet_last_error()
        self.qnet_pack = pkg.env.BatchedFourRoomEnv.qnet_pack.__get__(self)

    def close(self):
        self.lib.susnet_destroy(self._h)


def answers(pkg, env, m):
    """The five answers of one module, as the EXPECT rows list them."""
    P, T = pkg.policy, pkg.trainer.DeviceDQNTeamTrainer
    stack = P.linear_prelu_stack(m.model if isinstance(m, P.MLP) else m)
    net, dense, packed = P.DenseQNet(None, m), P.dense_stack(m), P.pack_mlp(env, m, ["onehot_pos"])
    return (stack and stack[2], net and net.dims, T._mlp_dims(m), dense and dense[2], packed and list(packed.dims))


def test_the_table_covers_what_it_should(pkg):
    assert sorted(_modules(pkg)) == sorted(EXPECT) and pkg._lib.MLP_MAX_F == 1024 and (pkg._lib.MLP_MAX_HIDDEN, pkg._lib.MLP_MAX_OUT) == (256, 32)


def test_every_caller_keeps_its_accept_set(pkg):
    env = _PackEnv(pkg)
    try:
        for name, m in _modules(pkg).items():
            assert answers(pkg, env, m) == EXPECT[name], name
    finally:
        env.close()


def test_the_recogniser_returns_the_layers_it_was_given(pkg):
    P = pkg.policy
    m = P.MLP(BASE)
    linears, acts, dims = P.linear_prelu_stack(m.model)
    assert [id(x) for x in linears] == [id(x) for x in list(m.model)[0::2]] and [id(x) for x in acts] == [id(x) for x in list(m.model)[1::2]]
    assert dims == BASE and P._mlp_stack(m)[2] == BASE and P._mlp_stack(m.model) is None
    # the two switches only widen: what they let through beyond the default is exactly the trailing activation and the unchained widths
    mods = _modules(pkg)
    for name, m in mods.items():
        seq = m.model if isinstance(m, P.MLP) else m
        loose = P.linear_prelu_stack(seq, chained=False, trailing_act=True)
        assert (loose is not None) == (EXPECT[name][0] is not None or name in ("trailing_activation", "unchained_width")), name
    assert len(P.linear_prelu_stack(mods["trailing_activation"].model, trailing_act=True)[1]) == 5


def test_the_dense_bounds_are_stated_once(pkg):
    P, L = pkg.policy, pkg._lib
    ok = P.stack_within_bounds
    assert ok([5000, 256, 32]) and not ok([5000, 256, 32], L.MLP_MAX_F) and not ok([0, 8, 4], L.MLP_MAX_F) and ok([1, 8, 4], 1)
    assert ok([8] * 8) and not ok([8] * 9) and ok([8, 32]) and not ok([8, 33]) and not ok([8, 0]) and not ok([8, 257, 4]) and not ok([8, 0, 4])


def _spatial(pkg, **over):
    cfg = dict(input_image_size=9, non_spatial_input_size=8, n_channels=[5, 6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1],
               rnn_layers=2, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[16], n_actions=6)
    cfg.update(over)
    return pkg.policy.SpatialDQN(**cfg)


def test_the_spatial_head_keeps_its_accept_set(pkg):
    P = pkg.policy
    mismatch = _spatial(pkg)
    mismatch.prediction_head[0] = nn.Linear(17, 16)  # in_features != rnn.hidden_size
    unchained = _spatial(pkg, mlp_hidden_layer_dims=[16, 12])
    unchained.prediction_head[2] = nn.Linear(20, 12)
    trailing = _spatial(pkg)
    trailing.prediction_head = nn.Sequential(*trailing.prediction_head, nn.PReLU())
    # name: (module, the head dims SpatialQNet serves or None): the parent's answers
    table = {
        "head_7": (_spatial(pkg, mlp_hidden_layer_dims=[8] * 6), [16] + [8] * 6 + [6]),
        "head_8": (_spatial(pkg, mlp_hidden_layer_dims=[8] * 7), None),
        "head_256": (_spatial(pkg, mlp_hidden_layer_dims=[256], rnn_layers=1), [16, 256, 6]),
        "head_256_two_rnn_layers": (_spatial(pkg, mlp_hidden_layer_dims=[256]), None),  # (SpatialQNet's own LDS rule, not the stack's)
        "head_257": (_spatial(pkg, mlp_hidden_layer_dims=[257]), None),
        "head_in_mismatch": (mismatch, None),
        "head_unchained": (unchained, None),
        "head_trailing_activation": (trailing, None),
    }
    for name, (m, dims) in table.items():
        net, stack = P.SpatialQNet(None, m), P._spatial_stack(m)
        assert (net and net.dims) == dims, name
        # the recogniser declines the malformed heads; the too-long and too-wide ones are recognised and then out of bounds
        assert (stack is None) == (name in ("head_in_mismatch", "head_unchained", "head_trailing_activation")), name
