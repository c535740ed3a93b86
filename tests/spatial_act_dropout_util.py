"""Shared by the tests of ACTING under dropout between the SpatialDQN's RNN layers (susnet_spatial_forward_dropout,
susnet_spatial_act_dropout_mask): include/susnet.h's statement of the acting mask restated in Python integers, the library's masks read
back, the dropout call through the C ABI on make_net-style networks (tests/spatial_exact.py), and the float64 restatement of such a
network's forward GIVEN its masks.  Nothing here is imported by a test that existed before these."""
import ctypes as C
import math

import numpy as np
import torch

from spatial_exact import CANARY, conv64, padded

SEED = 1  # the one mask seed of these tests: statements about "another offset / net gives other rows" are statements about THIS seed


def philox4x32_10(key, ctr):
    """Philox4x32-10 on one counter block (Salmon et al., SC'11), in Python integers."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def header_multiplier(p, seed, offset, net, agent, g, t, layer, unit):
    """include/susnet.h's m(net, agent, row G, t, layer, unit), restated: 0 or 1 / (1 - p) in float32."""
    p32 = float(np.float32(p))
    ctr = (unit // 4 | layer << 8 | t << 12 | net << 16 | agent << 20, g & 0xFFFFFFFF, (g >> 32) & 0xFF | (offset >> 32) << 8, offset & 0xFFFFFFFF)
    word = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), ctr)[unit % 4]
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if word >= math.floor(p32 * 2.0 ** 32) else 0.0


def header_act_mask(p, seed, offset, net, agents, row_base, layers, n, T, H):
    """The acting mask [layers - 1, n, T, H] by the header's mapping: row r is (agent r % agents, row G = row_base + r // agents)."""
    out = np.zeros((layers - 1, n, T, H), dtype=np.float32)
    for l in range(layers - 1):
        for r in range(n):
            for t in range(T):
                for u in range(H):
                    out[l, r, t, u] = header_multiplier(p, seed, offset, net, r % agents, row_base + r // agents, t, l, u)
    return out


def make_act_drop(L, p, net, seed=SEED, offset=0, row_base=0):
    """A susnet_rnn_dropout for an acting call of ``net`` (2 / 3): p goes where that net reads it, the other p is poisoned (not looked at)."""
    d = L.RnnDropout()
    d.p[net - 2], d.p[3 - net] = p, 7.0
    d.seed, d.offset, d.row_base = seed, offset, row_base
    return d


def export_act_mask(pkg, env, drop, net, agents, layers, n, T, H):
    """susnet_spatial_act_dropout_mask: float32 [layers - 1, n, T, H] on the host, canaries around the device buffer checked."""
    L = pkg._lib
    total = (layers - 1) * n * T * H
    buf = torch.full((total + 64,), -7.0, dtype=torch.float32, device=env.device)
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_spatial_act_dropout_mask(env._h, C.byref(drop), net, agents, layers, n, T, H, buf.data_ptr() + 32 * 4, env._stream()))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:32] == -7.0).all() and (out[32 + total:] == -7.0).all(), "susnet_spatial_act_dropout_mask wrote outside out"
    return out[32:32 + total].reshape(layers - 1, n, T, H).copy()


def net_io(pkg, net, dev, spatial, sp_strides, non_spatial, ns_strides, agents, n, T, rnn_in, q_out):
    """The susnet_spatial_io of a make_net-style network (``dev``: spatial_exact.upload's device tensors) on one call's buffers."""
    L = pkg._lib
    io = L.SpatialIO()
    io.T, io.N, io.C, io.n_conv, io.k, io.Fn = T, net["N"], net["C"], len(net["convs"]), net["k"], net["Fn"]
    for l, (co, s, p, d) in enumerate(net["convs"]):
        io.conv_out[l], io.conv_stride[l], io.conv_padding[l], io.conv_dilation[l] = co, s, p, d
        io.conv_weight[l], io.conv_bias[l] = dev["cw"][l].data_ptr(), dev["cb"][l].data_ptr()
    io.rnn_layers, io.rnn_hidden = net["L"], net["H"]
    for l in range(net["L"]):
        io.w_ih[l], io.w_hh[l], io.b_ih[l], io.b_hh[l] = (dev[k][l].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
    io.n_dims = len(net["dims"])
    for i, d in enumerate(net["dims"]):
        io.dims[i] = d
    for l in range(len(net["hw"])):
        io.weight[l], io.bias[l] = dev["hw"][l].data_ptr(), dev["hb"][l].data_ptr()
    for l in range(len(net["hw"]) - 1):
        io.slope[l] = dev["slope"][l].data_ptr()
    io.spatial, io.non_spatial = spatial.data_ptr(), non_spatial.data_ptr()
    for d in range(3):
        io.spatial_stride[d], io.non_spatial_stride[d] = sp_strides[d], ns_strides[d]
    io.agents, io.n, io.rnn_in, io.q_out = agents, n, rnn_in.data_ptr(), q_out.data_ptr()
    return io


def forward_net(pkg, env, net, dev, inp, n, T, drop=None, act_net=2):
    """One call on exact_inputs' arrays ``inp`` (spatial_exact.py) between canaries: susnet_spatial_forward_dropout with ``drop`` as
    ``act_net``, or susnet_spatial_forward where ``drop`` is None.  -> q [n, n_out] float32 on the host."""
    L = pkg._lib
    sp_buf, sp = padded(inp["sp_shape"], 3)
    sp.copy_(torch.from_numpy(inp["x"].astype(np.float32)))
    ns_buf, nsd = padded(inp["ns_shape"], 5)
    if net["Fn"]:
        nsd.copy_(torch.from_numpy(inp["ns"].astype(np.float32)))
    in_buf, rnn_in = padded((n, T, net["R"]), 7)
    q_buf, q = padded((n, net["dims"][-1]), 5)
    io = net_io(pkg, net, dev, sp, inp["sp_strides"], nsd, inp["ns_strides"], inp["A"], n, T, rnn_in, q)
    with torch.cuda.device(env.device):
        if drop is None:
            L.check(env.lib.susnet_spatial_forward(env._h, C.byref(io), env._stream()))
        else:
            L.check(env.lib.susnet_spatial_forward_dropout(env._h, C.byref(io), C.byref(drop), act_net, env._stream()))
    torch.cuda.synchronize()
    for buf, pad in ((in_buf, 7), (q_buf, 5)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), "canary"
    return q.cpu().numpy()


def masked_evaluate64(net, images, ns, masks):
    """An EXACT (integer) make_net network's forward under ``masks`` [L - 1][n, T, H] in float64: images [n, T, C, N, N], ns [n, T, Fn] ->
    q [n, n_out] as float32 holding the exact values.  Asserted on the way, as spatial_exact.evaluate64 does: every RNN pre-activation is a
    multiple of 32 (so tanh is exactly 0 / +-1 -- the masks must then be 0 / 2.0, p = 0.5) and every value float32 holds exactly."""
    assert not net.get("real", False)
    n, T = images.shape[:2]
    x = images.reshape(n * T, *images.shape[2:])
    for (co, s, p, d), W, b in zip(net["convs"], net["cw"], net["cb"]):
        x = conv64(x, W, b, s, p, d)
    rnn_in = np.concatenate([x.reshape(n, T, -1), ns], axis=2)
    H, L = net["H"], net["L"]
    h = [np.zeros((n, H)) for _ in range(L)]
    for t in range(T):
        below = rnn_in[:, t]
        for l in range(L):
            w_ih, w_hh, b_ih, b_hh = (net[key][l] for key in ("w_ih", "w_hh", "b_ih", "b_hh"))
            mag = np.abs(below) @ np.abs(w_ih).T + np.abs(h[l]) @ np.abs(w_hh).T + np.abs(b_ih) + np.abs(b_hh)
            z = below @ w_ih.T + h[l] @ w_hh.T + b_ih + b_hh
            assert float(mag.max()) < 2.0 ** 24 and np.array_equal(z, np.round(z / 32.0) * 32.0), "every pre-activation is a multiple of 32"
            h[l] = np.tanh(z)
            assert np.isin(h[l], (-1.0, 0.0, 1.0)).all()
            below = h[l] * masks[l][:, t].astype(np.float64) if l < L - 1 else h[l]  # (the layer's own recurrence keeps the undropped h)
    z = h[-1]
    for l, (W, b) in enumerate(zip(net["hw"], net["hb"])):
        z = z @ W.T + b
        if l < len(net["hw"]) - 1:
            z = np.where(z > 0, z, net["slopes"][l] * z)
    want = z.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), z) and float(np.abs(z).max()) < 2.0 ** 20
    return want


# ---- torch modules on the featurizers' layouts -------------------------------------------------------------------------------------------
def layout_inputs(rng, layout, B, T, A, C_in, N, Fn):
    """0/1 planes and non-spatial rows as a featurizer lays them out -- "global": spatial [B, T, C, N, N] (agent stride 0), "perspective":
    [B, T, A, C, N, N]; non_spatial [B, T, A, Fn] either way -- and the same per row r = b A + i: rows_x [n, T, C, N, N], rows_ns [n, T, Fn]."""
    ns = (rng.random((B, T, A, Fn)) < 0.5).astype(np.float32)
    if layout == "global":
        x = (rng.random((B, T, C_in, N, N)) < 0.3).astype(np.float32)
        rows_x = np.repeat(x[:, None], A, axis=1).reshape(B * A, T, C_in, N, N)
    else:
        x = (rng.random((B, T, A, C_in, N, N)) < 0.3).astype(np.float32)
        rows_x = x.transpose(0, 2, 1, 3, 4, 5).reshape(B * A, T, C_in, N, N)
    return x, ns, rows_x, ns.transpose(0, 2, 1, 3).reshape(B * A, T, Fn)
