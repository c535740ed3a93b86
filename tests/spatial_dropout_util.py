"""Shared by the tests of dropout between the SpatialDQN's RNN layers: the restatement of a training-mode ``SpatialDQN`` forward GIVEN its
masks (torch ops in the module's dtype, so autograd runs through it), the train step on it, and the library's masks read back.

What nn.RNN(num_layers=L, dropout=p, batch_first=True) computes in training mode (tests/golden/generate_spatial_dropout.py pins this to the
reference's module, test_spatial_dropout_host.py checks it): the output sequence of every layer l < L - 1 is multiplied elementwise by
m_l and the product feeds layer l + 1 only; layer l's own recurrence reads the undropped h_l; the last layer's output is not dropped."""
import copy
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F


def masked_rnn(rnn, x, masks):
    """``x`` [n, T, R] through ``rnn`` (nn.RNN, tanh, batch_first) with ``masks`` [L - 1][n, T, H] (None or empty: no dropout): the top
    layer's hidden state at the last step [n, H]."""
    n, T, _ = x.shape
    L, H = rnn.num_layers, rnn.hidden_size
    seq = [x[:, t] for t in range(T)]
    for l in range(L):
        w_ih, w_hh = getattr(rnn, f"weight_ih_l{l}"), getattr(rnn, f"weight_hh_l{l}")
        b = getattr(rnn, f"bias_ih_l{l}") + getattr(rnn, f"bias_hh_l{l}")
        h = torch.zeros(n, H, dtype=x.dtype)
        out = []
        for t in range(T):
            h = torch.tanh(seq[t] @ w_ih.T + h @ w_hh.T + b)  # (the recurrence reads the undropped h)
            out.append(h)
        if l < L - 1 and masks is not None and len(masks):
            seq = [out[t] * masks[l][:, t] for t in range(T)]  # (what layer l + 1 reads)
        else:
            seq = out
    return seq[-1]


def masked_forward(model, spatial, non_spatial, masks):
    """Q rows [n, n_actions] of ``spatial`` [n, T, C, N, N] and ``non_spatial`` [n, T, Fn] (dqn.py:275-293) with the RNN under ``masks``."""
    n, T = spatial.shape[:2]
    feats = model.cnn(spatial.reshape(n * T, *spatial.shape[2:])).reshape(n, T, -1)
    return model.prediction_head(masked_rnn(model.rnn.model, torch.cat((feats, non_spatial), dim=2), masks))


def masked_train_step(models, targets, optimizers, gamma, state_feats, next_state_feats, actions, rewards, dones, imposters, masks):
    """``torch_train_step`` (DQNTeamTrainer.train_step, train.py:50-149) with the forwards restated under given masks:
    ``masks[(agent, team)] = (online, target)``, each [L - 1][n, T, H] over ALL batch rows (row = the position in the batch; the rows of
    the update's list are selected here) or None."""
    losses = [0.0, 0.0]
    for opt in optimizers:
        if opt is not None:
            opt.zero_grad()
    for agent, (sf, nf) in enumerate(zip(state_feats, next_state_feats)):
        imp_rows = (imposters == agent).view(-1)
        for team, rows in ((0, imp_rows), (1, ~imp_rows)):
            opt, model, target = optimizers[team], models[team], targets[team]
            if opt is None or int(rows.sum()) == 0:
                continue
            on, tg = masks.get((agent, team), (None, None))
            pick = lambda m: None if m is None else [x[rows] for x in m]
            q = masked_forward(model, sf[0][rows], sf[1][rows], pick(on))
            values = torch.gather(q, 1, actions[rows, agent].view(-1, 1)).view(-1)
            with torch.no_grad():
                done_mask = dones[rows].view(-1)
                r = rewards[rows, agent].view(-1)
                y = r + gamma * torch.max(masked_forward(target, nf[0][rows], nf[1][rows], pick(tg)), dim=1)[0]
                y[done_mask] = r[done_mask]
            loss = F.mse_loss(values, y)
            loss.backward()
            losses[team] += loss.item()
            opt.step()
    return losses


def make_drop(L, p_online, p_target=0.0, seed=1, offset=0, row_base=0):
    d = L.RnnDropout()
    d.p[0], d.p[1], d.seed, d.offset, d.row_base = p_online, p_target, seed, offset, row_base
    return d


def export_mask(pkg, env, drop, net, agent, layers, n, T, H):
    """susnet_rnn_dropout_mask: float32 [layers - 1, n, T, H] on the host, canaries around the device buffer checked."""
    L = pkg._lib
    total = (layers - 1) * n * T * H
    buf = torch.full((total + 64,), -7.0, dtype=torch.float32, device=env.device)
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_rnn_dropout_mask(env._h, C.byref(drop), net, agent, layers, n, T, H, buf.data_ptr() + 32 * 4, env._stream()))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:32] == -7.0).all() and (out[32 + total:] == -7.0).all(), "susnet_rnn_dropout_mask wrote outside out"
    return out[32:32 + total].reshape(layers - 1, n, T, H).copy()


def library_masks(pkg, env, models, drops, n, T, A):
    """masks[(agent, team)] = (online, target), each [L - 1][n, T, H] float64 read back from the library (row = the position in the batch);
    (None, None) for a team with one RNN layer.  drops: [imposter, crew] susnet_rnn_dropout."""
    out = {}
    for agent in range(A):
        for team, m in enumerate(models):
            if m is None:
                continue
            rnn = m.rnn.model
            if rnn.num_layers < 2:
                out[agent, team] = (None, None)
                continue
            get = lambda net: list(torch.as_tensor(export_mask(pkg, env, drops[team], net, agent, rnn.num_layers, n, T, rnn.hidden_size)).double())
            out[agent, team] = (get(0), get(1))
    return out


def masked_reference(models, targets, batch, gamma, lr, masks, dtype=torch.float64):
    """One masked_train_step on CPU copies in ``dtype`` (the multipliers are exact in float32: 0 or 1 / (1 - p) rounded once by the library):
    (losses [2], exp_avg per team as flat float64, Adam step counts)."""
    from spatial_train_util import agent_feats

    ms = [m and copy.deepcopy(m).cpu().to(dtype) for m in models]
    ts = [t and copy.deepcopy(t).cpu().to(dtype) for t in targets]
    opts = [m and torch.optim.Adam(m.parameters(), lr=lr) for m in ms]
    cast = lambda m: None if m is None else [x.to(dtype) for x in m]
    masks = {k: (cast(on), cast(tg)) for k, (on, tg) in masks.items()}
    idx = torch.as_tensor(batch["idx"])
    sf, nf = agent_feats(batch, "spatial", dtype), agent_feats(batch, "next_spatial", dtype)
    losses = masked_train_step(ms, ts, opts, gamma, sf, nf, torch.as_tensor(batch["actions"])[idx].long(),
                               torch.as_tensor(batch["rewards"])[idx].to(dtype), torch.as_tensor(batch["dones"])[idx].bool().reshape(-1, 1),
                               torch.as_tensor(batch["imposters"])[idx].to(torch.int16).reshape(-1, 1), masks)
    ea, counts = [], []
    for m, o in zip(ms, opts):
        if m is None:
            ea.append(None), counts.append(0.0)
            continue
        ea.append(np.concatenate([(o.state[p]["exp_avg"].double().numpy().reshape(-1) if p in o.state else np.zeros(p.numel())) for p in m.parameters()]))
        counts.append(float(next(iter(o.state.values()))["step"]) if o.state else 0.0)
    return np.asarray(losses, dtype=np.float64), ea, counts
