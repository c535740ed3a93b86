"""Shared by the tests of the SpatialDQN train step (susnet_spatial_train_step): hand-made batches in both featurizer layouts, the C ABI
call by hand with canaries around everything it writes, and the float64 / float32 torch references (torch_train_step on CPU copies)."""
import copy
import ctypes as C

import numpy as np
import torch

from train_exact import BETAS, CANARY, DEV, EPS, Guarded, _workspace


def make_model(pkg, N, C_in, Fn, chans, strides, pads, k, dils, layers, hidden, head, n_actions, seed, dropout=0.0):
    """A SpatialDQN whose CNN has ``len(chans) + 1`` convolutions of widths ``chans + [chans[-1]]`` (the reference repeats the last entry of
    every list, dqn.py:155-159; ``chans = []`` is ONE convolution C_in -> C_in), distinct PReLU slopes, seeded."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = pkg.SpatialDQN(N, Fn, [C_in] + list(chans), strides, pads, (k, k), dils, layers, hidden, dropout, head, n_actions)
        with torch.no_grad():
            for i, act in enumerate(a for a in m.prediction_head if isinstance(a, torch.nn.PReLU)):
                act.weight.fill_(0.1 + 0.2 * i)
    return m


def tensors(model):
    """[(name, shape)] in parameters() order: the flat layout the step reads."""
    return [(n, tuple(p.shape)) for n, p in model.named_parameters()]


def flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).double().numpy()


def split(model, flat_values):
    out, off = [], 0
    for name, shape in tensors(model):
        n = int(np.prod(shape))
        out.append((name, np.asarray(flat_values[off:off + n]).reshape(shape)))
        off += n
    assert off == len(flat_values)
    return out


def make_batch(rng, n, T, A, C_in, N, Fn, n_actions, M=None, density=0.3):
    """0/1 planes and 0/1 non-spatial rows PER AGENT ([n, T, A, ..]: the Perspective layout), ring arrays of M rows."""
    M = M or n + 5
    plane = lambda: (rng.random((n, T, A, C_in, N, N)) < density).astype(np.float32)
    feat = lambda: (rng.random((n, T, A, Fn)) < 0.5).astype(np.float32)
    return dict(spatial=plane(), next_spatial=plane(), non_spatial=feat(), next_non_spatial=feat(), idx=rng.integers(0, M, n).astype(np.int64),
                actions=rng.integers(0, n_actions, (M, A)), rewards=rng.normal(size=(M, A)).astype(np.float32),
                dones=(rng.random(M) < 0.3).astype(np.uint8), imposters=rng.integers(0, A, M).astype(np.int16))


def as_global(batch):
    """The same batch in the Global featurizer's layout: every agent reads agent 0's planes ([n, T, C, N, N], agent stride 0); the
    non-spatial rows stay per agent (the Global featurizer appends the agent's one-hot)."""
    out = dict(batch)
    out["spatial"], out["next_spatial"] = batch["spatial"][:, :, 0].copy(), batch["next_spatial"][:, :, 0].copy()
    return out


def agent_feats(batch, key, dtype):
    """[(spatial [n, T, C, N, N], non_spatial [n, T, Fn])] per agent, as generate_featurized_states() returns them."""
    sp, ns = torch.as_tensor(batch[key]).to(dtype), torch.as_tensor(batch[key.replace("spatial", "non_spatial")]).to(dtype)
    A = ns.shape[2]
    return [(sp if sp.dim() == 5 else sp[:, :, i], ns[:, :, i]) for i in range(A)]


def torch_reference(pkg, models, targets, batch, gamma, lr, dtype, steps=1):
    """``steps`` torch_train_step calls on CPU copies in ``dtype``: (losses per step [steps][2], exp_avg per team as flat float64, Adam step
    counts, flat parameters per team).  models / targets: [imposter, crew], None = the team does not train."""
    ms = [m and copy.deepcopy(m).to(dtype) for m in models]
    ts = [t and copy.deepcopy(t).to(dtype) for t in targets]
    opts = [m and torch.optim.Adam(m.parameters(), lr=lr) for m in ms]
    idx = torch.as_tensor(batch["idx"])
    sf, nf = agent_feats(batch, "spatial", dtype), agent_feats(batch, "next_spatial", dtype)
    losses = []
    for _ in range(steps):
        losses.append(pkg.torch_train_step(ms, ts, opts, gamma, sf, nf, torch.as_tensor(batch["actions"])[idx].long(),
                                           torch.as_tensor(batch["rewards"])[idx].to(dtype), torch.as_tensor(batch["dones"])[idx].bool().reshape(-1, 1),
                                           torch.as_tensor(batch["imposters"])[idx].to(torch.int16).reshape(-1, 1)))
    ea, counts, params = [], [], []
    for m, o in zip(ms, opts):
        if m is None:
            ea.append(None), counts.append(0.0), params.append(None)
            continue
        ea.append(np.concatenate([(o.state[p]["exp_avg"].double().numpy().reshape(-1) if p in o.state else np.zeros(p.numel())) for p in m.parameters()]))
        counts.append(float(next(iter(o.state.values()))["step"]) if o.state else 0.0)
        params.append(flat(m))
    return np.asarray(losses, dtype=np.float64), ea, counts, params


def fill_net(net, model, T):
    """susnet_spatial_net of a SpatialDQN."""
    convs = [m for m in model.cnn.model if isinstance(m, torch.nn.Conv2d)]
    rnn = model.rnn.model
    net.T, net.N, net.C, net.Fn = T, model.config["input_image_size"], convs[0].in_channels, model.config["non_spatial_input_size"]
    net.n_conv, net.k = len(convs), convs[0].kernel_size[0]
    for l, m in enumerate(convs):
        net.conv_out[l], net.conv_stride[l], net.conv_padding[l], net.conv_dilation[l] = m.out_channels, m.stride[0], m.padding[0], m.dilation[0]
    net.rnn_layers, net.rnn_hidden = rnn.num_layers, rnn.hidden_size


class SpatialCall:
    """One susnet_spatial_train_io by hand on a batch of make_batch / as_global, device buffers with canaries, the Adam state carried in
    the object: ``step()`` may be called again.  models / targets: [imposter, crew] modules (None: the team is not enabled)."""

    def __init__(self, pkg, env, models, targets, batch, gamma, lr=1e-3, betas=BETAS):
        L = pkg._lib
        self.pkg, self.env, self.models, self.batch = pkg, env, models, batch
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
        io = self.io = L.SpatialTrainIO()
        n = len(batch["idx"])
        sp = batch["spatial"]
        T, A = sp.shape[1], batch["non_spatial"].shape[2]
        Fn = batch["non_spatial"].shape[3]
        self.keep = [dev(batch[k], torch.float32) for k in ("spatial", "next_spatial", "non_spatial", "next_non_spatial")]
        self.keep += [dev(batch["idx"], torch.int64), dev(batch["actions"], torch.int64), dev(batch["rewards"], torch.float32),
                      dev(batch["dones"], torch.uint8), dev(batch["imposters"].reshape(-1, 1), torch.int16)]
        s, ns_, x, nx, idx, actions, rewards, dones, imposters = self.keep
        io.spatial, io.next_spatial = s.data_ptr(), ns_.data_ptr()
        io.non_spatial, io.next_non_spatial = (x.data_ptr(), nx.data_ptr()) if Fn > 0 else (None, None)
        img = int(np.prod(sp.shape[-3:]))
        strides = (T * A * img, img, A * img) if sp.ndim == 6 else (T * img, 0, img)
        for d in range(3):
            io.spatial_stride[d], io.non_spatial_stride[d] = strides[d], (T * A * Fn, Fn, A * Fn)[d]
        io.indices, io.n = (idx.data_ptr() if n else None), n
        io.actions, io.rewards, io.dones, io.imposters = actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(), imposters.data_ptr()
        io.max_size, io.gamma = actions.shape[0], gamma
        self.bufs = [None, None]
        for t, (m, tg) in enumerate(zip(models, targets)):
            if m is None:
                continue
            P = sum(p.numel() for p in m.parameters())
            g = dict(params=Guarded(flat(m)), target=Guarded(flat(tg)), exp_avg=Guarded(n=P), exp_avg_sq=Guarded(n=P),
                     step=torch.zeros(1, dtype=torch.float32, device=DEV))
            self.bufs[t] = g
            tm = io.team[t]
            dims = [m.rnn.model.hidden_size] + [l.out_features for l in m.prediction_head if isinstance(l, torch.nn.Linear)]
            tm.enabled, tm.n_dims = 1, len(dims)
            for k, d in enumerate(dims):
                tm.dims[k] = d
            tm.lr, tm.beta1, tm.beta2, tm.eps = lr, betas[0], betas[1], EPS
            tm.params, tm.target_params = g["params"].ptr(), g["target"].ptr()
            tm.exp_avg, tm.exp_avg_sq, tm.step = g["exp_avg"].ptr(), g["exp_avg_sq"].ptr(), g["step"].data_ptr()
            fill_net(io.net[t], m, T)
        self.losses = torch.full((4,), CANARY, dtype=torch.float32, device=DEV)  # [canary, imposter, crew, canary]
        io.losses_out = self.losses.data_ptr() + 4
        nbytes = C.c_uint64()
        L.check(env.lib.susnet_spatial_train_workspace_bytes(env._h, C.byref(io), C.byref(nbytes)))
        self.nbytes = int(nbytes.value)
        self.ws = _workspace(self.nbytes)
        io.workspace, io.workspace_bytes = self.ws.data_ptr(), self.nbytes

    def launch(self):
        """The call alone (what a graph captures)."""
        self.pkg._lib.check(self.env.lib.susnet_spatial_train_step(self.env._h, C.byref(self.io), self.env._stream()))

    def step(self):
        with torch.cuda.device(DEV):
            self.launch()
        torch.cuda.synchronize()
        return self.results()

    def results(self):
        """(losses [2], per team dict of float64 params / exp_avg / exp_avg_sq, step and the raw float32 bits)."""
        lo = self.losses.cpu().numpy()
        assert lo[0] == CANARY and lo[3] == CANARY, "losses_out: a neighbour was written"
        assert bool((self.ws[self.nbytes:] == 0x5A).all()), "the workspace was overrun"
        out = [None, None]
        for t, g in enumerate(self.bufs):
            if g is None:
                continue
            for k in ("params", "target", "exp_avg", "exp_avg_sq"):
                assert g[k].intact(), f"team {t} {k}: a canary was overwritten"
            out[t] = dict(params=g["params"].numpy(), exp_avg=g["exp_avg"].numpy(), exp_avg_sq=g["exp_avg_sq"].numpy(), step=float(g["step"]),
                          bits=[g[k].view.cpu().numpy().copy() for k in ("params", "exp_avg", "exp_avg_sq")] + [g["step"].cpu().numpy().copy()])
        return lo[1:3].astype(np.float64), out


def compare_tensors(model, got, ref, ref32, what, tol=1e-4):
    """Every parameter tensor on its own: ``got`` within ``tol`` of the tensor's max-abs of ``ref``; ``ref32``'s own error printed beside it."""
    worst = 0.0
    for (name, g_), (_, r_), (_, f_) in zip(split(model, got), split(model, ref), split(model, ref32)):
        peak = float(np.abs(r_).max())
        scale = max(peak, 1e-30)
        err, err32 = float(np.abs(g_ - r_).max()) / scale, float(np.abs(f_ - r_).max()) / scale
        print(f"{what} {name}: kernel {err:.2e}, float32 torch {err32:.2e} of max-abs {peak:.3e}")
        assert err <= tol or peak == 0.0 == float(np.abs(g_).max()), f"{what} {name}: off by {err:.2e} of max-abs (float32 torch: {err32:.2e})"
        worst = max(worst, err)
    return worst
