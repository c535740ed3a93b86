#!/usr/bin/env python3
"""Golden vectors for dropout between the SpatialDQN's RNN layers (container only): the UNMODIFIED reference `SpatialDQN`
(src/models/dqn.py:205-301) in TRAINING mode on the CPU in float64, on inputs of the Global featurizer's shapes at 9x9 (1v4: 7 planes, 15
non-spatial columns), n = 5 rows, T = 3.  Stored as data: the parameters by state_dict key, the inputs, the dropout masks torch drew and
the module's training-mode outputs; for one case also the gradients of a sum of gathered Q values.

The masks are recovered, not injected: on the CPU nn.RNN in training mode draws, per layer l < L - 1 and in layer order, ONE mask over
that layer's whole output sequence in time-major order, `torch.empty(T, n, H).bernoulli_(1 - p).div_(1 - p)`; reseeding and drawing the
same way gives the same values.  That this is what happened is checked here before anything is written: the float64 restatement of
tests/spatial_dropout_util.py fed those masks must reproduce the module's outputs (and gradients) to 1e-12.

    python tests/golden/generate_spatial_dropout.py        # rewrites tests/golden/spatial_dropout/*.npz
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refshim  # noqa: E402

_refshim.install()
import torch  # noqa: E402

from spatial_dropout_util import masked_forward  # noqa: E402
from src.models.dqn import SpatialDQN  # noqa: E402

OUT = os.path.join(HERE, "spatial_dropout")
N, C, FN, ROWS, T, HIDDEN, ACTIONS = 9, 7, 15, 5, 3, 12, 5


def dump(name, layers, p, seed, with_gradients):
    cfg = dict(input_image_size=N, non_spatial_input_size=FN, n_channels=[C, 4, 3], strides=[1, 1], paddings=[1, 1], kernel_size=[3, 3],
               dilations=[1, 1], rnn_layers=layers, rnn_hidden_dim=HIDDEN, rnn_dropout=p, mlp_hidden_layer_dims=[6], n_actions=ACTIONS)
    torch.manual_seed(seed)
    model = SpatialDQN(**cfg).double()
    with torch.no_grad():
        for i, mod in enumerate(m for m in model.modules() if isinstance(m, torch.nn.PReLU)):
            mod.weight.fill_((0.1, 0.3)[i])
    rng = np.random.default_rng(seed)
    spatial = torch.tensor((rng.random((ROWS, T, C, N, N)) < 0.3).astype(np.float64))
    non_spatial = torch.tensor((rng.random((ROWS, T, FN)) < 0.5).astype(np.float64))
    actions = torch.tensor(rng.integers(0, ACTIONS, ROWS))
    model.train()
    torch.manual_seed(seed + 1)
    q = model(spatial, non_spatial)
    torch.manual_seed(seed + 1)
    masks = [torch.empty(T, ROWS, HIDDEN, dtype=torch.float64).bernoulli_(1 - p).div_(1 - p).transpose(0, 1).contiguous() for _ in range(layers - 1)]
    restated = masked_forward(model, spatial, non_spatial, masks)
    err = float((restated - q).detach().abs().max())
    assert err <= 1e-12, f"{name}: the recovered masks do not reproduce the module's training-mode output ({err:.2e})"
    assert float((masked_forward(model, spatial, non_spatial, None) - q).detach().abs().max()) > 1e-3, f"{name}: dropout changed nothing"
    arrays = {f"param::{k}": v.detach().numpy() for k, v in model.state_dict().items()}
    if with_gradients:
        model.zero_grad()
        torch.gather(q, 1, actions.view(-1, 1)).sum().backward()
        arrays.update({f"grad::{k}": v.grad.detach().numpy() for k, v in model.named_parameters()})
    meta = dict(config=cfg, layers=layers, p=p, seed=seed, rows=ROWS, T=T)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), spatial=spatial.numpy().astype(np.uint8), non_spatial=non_spatial.numpy().astype(np.uint8),
                        actions=actions.numpy(), masks=np.stack([m.numpy() for m in masks]), q=q.detach().numpy(), **arrays)
    print(name, "restatement off by", err, "bytes", os.path.getsize(path))


def main():
    dump("l2_p50", 2, 0.5, 41, False)
    dump("l3_p50", 3, 0.5, 42, True)
    dump("l2_p20", 2, 0.2, 43, False)
    dump("l3_p20", 3, 0.2, 44, False)


if __name__ == "__main__":
    main()
