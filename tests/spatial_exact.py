"""Shared by the tests of the SpatialDQN forward kernels (susnet_spatial_forward): integer-valued networks whose float64 evaluation every
float32 summation order reproduces (tanh pinned to 0 / +-1, head slopes signed powers of two or 0), real-valued networks with their float64
evaluation, the float32 error to expect of it and a float32 yardstick in the kernels' documented operation order, the documented tanh
formula in numpy, a restatement of the dispatch and LDS rules of DESIGN.md ("The SpatialDQN forward kernels"), the stack tables of the GPU
tests, and the calls through the C ABI.  Used by the CPU test of these helpers (test_spatial_exact_host.py) and the GPU tests
(test_gpu_spatial.py, test_gpu_spatial_limits.py); nothing here touches a GPU until a function that launches is called, and the package
is handed in."""
import ctypes as C
import zlib

import numpy as np
import torch

DEV = "cuda:0"
CANARY = 12345.0
U32 = 2.0 ** -24  # float32's unit roundoff


# ---- an integer-valued or real-valued network and its float64 evaluation ---------------------------------------------------------------
def conv_lin64(x, W, b, stride, pad, dil):
    """The Conv2d of x [M, Ci, H, H] before its ReLU, in float64."""
    K = W.shape[-1]
    H = x.shape[-1]
    Ho = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((x.shape[0], W.shape[0], Ho, Ho)) + b[None, :, None, None]
    for ky in range(K):
        for kx in range(K):
            patch = xp[:, :, ky * dil:ky * dil + stride * (Ho - 1) + 1:stride, kx * dil:kx * dil + stride * (Ho - 1) + 1:stride]
            out += np.einsum("mchw,oc->mohw", patch, W[:, :, ky, kx])
    return out


def conv64(x, W, b, stride, pad, dil):
    """Conv2d + ReLU in float64 on x [M, Ci, H, H]; asserts the bound max(sum |w||x| + |b|) < 2^24 that makes float32 exact in any order."""
    mag = conv_lin64(np.abs(x), np.abs(W), np.abs(b), stride, pad, dil)
    assert float(mag.max()) < 2.0 ** 24, float(mag.max())
    return np.maximum(conv_lin64(x, W, b, stride, pad, dil), 0.0)


REAL_SCALES = dict(conv=1.0, conv_b=0.1, w_ih0=1.5, w_ih=1.5, w_hh=1.0, b=0.5, head=1.5, head_b=0.2)


def make_net(rng, N, C, k, convs, Fn, L, H, head, variant=None, slopes=None, real=False, scales=None):
    """convs: [(out channels, stride, padding, dilation)].  Convolution and head parameters from {-1, 0, 1}, RNN weights and summed biases
    from {-32, 0, 32} (b_ih + b_hh: some as 16 + 16), head slopes ``slopes`` (one per hidden head layer; default 0.5 each).
    ``real=True``: every parameter a float32-representable normal draw, weights scaled by scales[part] / sqrt(fan-in) and biases by
    scales[part] (REAL_SCALES, overridden by ``scales``); ``slopes`` are then any real numbers."""
    net = dict(N=N, C=C, k=k, convs=convs, Fn=Fn, L=L, H=H, variant=variant, real=real)
    dims = net["dims"] = [H] + list(head)
    net["slopes"] = [0.5] * (len(dims) - 2) if slopes is None else [float(s) for s in slopes]
    assert len(net["slopes"]) == len(dims) - 2
    sc = dict(REAL_SCALES, **(scales or {}))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    draw = lambda shape, fan_in, part: f32(rng.standard_normal(shape) * sc[part] / np.sqrt(fan_in))
    ci, size = C, N
    net["cw"], net["cb"] = [], []
    for co, s, p, d in convs:
        if real:
            net["cw"].append(draw((co, ci, k, k), ci * k * k, "conv"))
            net["cb"].append(draw(co, 1, "conv_b"))
        else:
            net["cw"].append(rng.choice([-1.0, 0.0, 1.0], size=(co, ci, k, k), p=[0.25, 0.5, 0.25]))
            net["cb"].append(rng.choice([-1.0, 0.0, 1.0], size=co))
        size = (size + 2 * p - d * (k - 1) - 1) // s + 1
        ci = co
    net["conv_cols"] = ci * size * size
    R = net["R"] = net["conv_cols"] + Fn
    net["w_ih"], net["w_hh"], net["b_ih"], net["b_hh"] = [], [], [], []
    for l in range(L):
        if real:
            net["w_ih"].append(draw((H, R if l == 0 else H), R if l == 0 else H, "w_ih0" if l == 0 else "w_ih"))
            net["w_hh"].append(draw((H, H), H, "w_hh"))
            net["b_ih"].append(draw(H, 1, "b"))
            net["b_hh"].append(draw(H, 1, "b"))
            continue
        w_ih = rng.choice([-32.0, 0.0, 32.0], size=(H, R if l == 0 else H), p=[0.1, 0.8, 0.1])
        w_hh = rng.choice([-32.0, 0.0, 32.0], size=(H, H), p=[0.15, 0.7, 0.15])
        if variant == "no_recurrence":
            w_hh[:] = 0.0
        if variant == "carry" and l == 0:  # layer 0 reads the non-spatial columns only, and they are zero after t = 0: what the answer
            w_ih[:, :net["conv_cols"]] = 0.0  # knows of the input it knows through the recurrence
        b = rng.choice([-32.0, 0.0, 32.0], size=H)
        split = rng.random(H) < 0.3
        net["w_ih"].append(w_ih)
        net["w_hh"].append(w_hh)
        net["b_ih"].append(np.where(split, b / 2, b))
        net["b_hh"].append(np.where(split, b / 2, 0.0))
    if real:
        net["hw"] = [draw((dims[l + 1], dims[l]), dims[l], "head") for l in range(len(dims) - 1)]
        net["hb"] = [draw(dims[l + 1], 1, "head_b") for l in range(len(dims) - 1)]
    else:
        net["hw"] = [rng.choice([-1.0, 0.0, 1.0], size=(dims[l + 1], dims[l]), p=[0.3, 0.4, 0.3]) for l in range(len(dims) - 1)]
        net["hb"] = [rng.choice([-1.0, 0.0, 1.0], size=dims[l + 1]) for l in range(len(dims) - 1)]
    return net


def slope_denominator(s):
    """2^e such that multiplying a multiple of 1/den by slope s gives a multiple of 1 / (den 2^e); s is 0 or a signed power of two."""
    if s == 0.0:
        return 1.0
    m, e = np.frexp(abs(s))
    assert m == 0.5, f"slope {s}: exact networks take 0 and signed powers of two"
    return 2.0 ** max(0, 1 - int(e))


TANH_SIGMA_ULPS = 2.0  # the float32 tanh's own error as a standard deviation: three roundings behind expm1f, and expm1f's ulp times up to 2
SIGMAS = 6.0  # how many of evaluate64's standard deviations a float32 evaluation may be off, element by element


def evaluate64(net, images, ns, slopes=None, check=True):
    """images [n, T, C, N, N], ns [n, T, Fn] (float64); ``slopes`` replaces the net's.
    Exact networks -> (rnn_in [n, T, R], q [n, n_out]) as float32 arrays that hold the exact values; asserted on the way: every
    intermediate is a dyadic rational float32 holds, because every sum |w||x| + |b| times the common denominator stays below 2^24.
    Real networks -> dict(rnn_in, q: float64; pre [T, L, n, H]: the RNN's pre-activations; rnn_in_sigma, q_sigma: elementwise, the
    standard deviation a float32 evaluation's error is expected to stay within -- see the note in the body).
    ``check=False`` (exact networks): evaluate only, as float64 -- for asking whether another set of slopes changes the answer."""
    real = net.get("real", False) or not check
    slopes = net["slopes"] if slopes is None else slopes
    n, T = images.shape[:2]
    x = images.reshape(n * T, *images.shape[2:])
    # The expected float32 error (real mode).  A worst-case bound (Higham's gamma(K) sum |w||x| per chain, carried on through |W|) grows by
    # the 1-norm of every weight matrix at every layer and time step and says nothing after a recurrence.  The model here is the
    # probabilistic one (Higham & Mary, "A new approach to probabilistic rounding error analysis", SIAM J. Sci. Comput. 41, 2019): the
    # roundings are independent, of mean zero and at most u = 2^-24 relative, so a chain b + sum_k w_k x_k of K products (multiply and add
    # rounded separately; a fused multiply-add has fewer roundings) has an error of standard deviation at most sqrt(K + 1) u (sum |w||x| +
    # |b|), and errors of the operands with variances v_k add sum w_k^2 v_k.  An activation multiplies the error by its derivative (ReLU 0
    # or 1; tanh 1 - h^2; PReLU 1 or a) and adds its own rounding (PReLU's product: u |a z|; the float32 tanh: TANH_SIGMA_ULPS u |h|).
    # First order in u.  Tests allow SIGMAS times this.
    vx = np.zeros_like(x)
    for (co, s, p, d), W, b in zip(net["convs"], net["cw"], net["cb"]):
        if real:
            mag = conv_lin64(np.abs(x), np.abs(W), np.abs(b), s, p, d)
            vx = conv_lin64(vx, W * W, np.zeros_like(b), s, p, d) + (W[0].size + 1) * (U32 * mag) ** 2
            x = np.maximum(conv_lin64(x, W, b, s, p, d), 0.0)
        else:
            x = conv64(x, W, b, s, p, d)
    rnn_in = np.concatenate([x.reshape(n, T, -1), ns], axis=2)
    v_in = np.concatenate([vx.reshape(n, T, -1), np.zeros_like(ns)], axis=2)
    assert rnn_in.shape[2] == net["R"]
    H, L = net["H"], net["L"]
    h = [np.zeros((n, H)) for _ in range(L)]
    vh = [np.zeros((n, H)) for _ in range(L)]
    pre = np.zeros((T, L, n, H))
    for t in range(T):
        below, v_below = rnn_in[:, t], v_in[:, t]
        for l in range(L):
            w_ih, w_hh, b_ih, b_hh = (net[key][l] for key in ("w_ih", "w_hh", "b_ih", "b_hh"))
            mag = np.abs(below) @ np.abs(w_ih).T + np.abs(h[l]) @ np.abs(w_hh).T + np.abs(b_ih) + np.abs(b_hh)
            z = below @ w_ih.T + h[l] @ w_hh.T + b_ih + b_hh
            pre[t, l] = z
            if real:
                vz = v_below @ (w_ih * w_ih).T + vh[l] @ (w_hh * w_hh).T + (w_ih.shape[1] + H + 2) * (U32 * mag) ** 2
                h[l] = np.tanh(z)
                vh[l] = (1.0 - h[l] ** 2) ** 2 * vz + (TANH_SIGMA_ULPS * U32 * h[l]) ** 2
            else:
                assert float(mag.max()) < 2.0 ** 24
                assert np.array_equal(z, np.round(z / 32.0) * 32.0), "every pre-activation is a multiple of 32"
                h[l] = np.tanh(z)
                assert np.isin(h[l], (-1.0, 0.0, 1.0)).all()
            below, v_below = h[l], vh[l]
    z, vz, den = h[-1], vh[-1], 1.0
    for l, (W, b) in enumerate(zip(net["hw"], net["hb"])):
        mag = np.abs(z) @ np.abs(W).T + np.abs(b)
        if real:
            vz = vz @ (W * W).T + (W.shape[1] + 1) * (U32 * mag) ** 2
        else:
            assert float(mag.max()) * den < 2.0 ** 24, (l, float(mag.max()), den)
        z = z @ W.T + b
        if l < len(net["hw"]) - 1:
            a = slopes[l]
            if real:
                vz = np.where(z > 0, vz, a * a * vz + (U32 * a * z) ** 2)
            else:
                den *= slope_denominator(a)
            z = np.where(z > 0, z, a * z)
            if not real:
                assert np.array_equal(z * den, np.round(z * den)) and float(np.abs(z).max()) * den < 2.0 ** 24, (l, a, den)
    if real:
        return dict(rnn_in=rnn_in, q=z, pre=pre, rnn_in_sigma=np.sqrt(v_in), q_sigma=np.sqrt(vz))
    want_in, want_q = rnn_in.astype(np.float32), z.astype(np.float32)
    assert np.array_equal(want_in.astype(np.float64), rnn_in) and np.array_equal(want_q.astype(np.float64), z)
    return want_in, want_q


# ---- the documented float32 evaluation, restated -------------------------------------------------------------------------------------------
def tanh_formula32(x):
    """susnet_spatial.h's tanh in numpy float32 with an accurate expm1: e = expm1(-2 |x|) rounded to float32, t = -e / (e + 2), 1 where
    |x| >= 16, the sign copied from x."""
    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    with np.errstate(over="ignore"):
        arg = (np.float32(-2.0) * ax).astype(np.float32)
    e = np.expm1(arg.astype(np.float64)).astype(np.float32)
    t = (-e / (e + np.float32(2.0)).astype(np.float32)).astype(np.float32)
    t = np.where(ax >= np.float32(16.0), np.float32(1.0), t).astype(np.float32)
    return np.copysign(t, x).astype(np.float32)


def chain32(acc, W, X):
    """acc [m, n_out] (float32) + sum_k X[:, k] W[:, k], one chain over k ascending, every multiply and every add rounded to float32."""
    W, X = np.ascontiguousarray(W.T, dtype=np.float32), np.ascontiguousarray(X.T, dtype=np.float32)
    for k in range(W.shape[0]):
        acc = acc + X[k][:, None] * W[k][None, :]  # float32 * float32 and float32 + float32: numpy rounds each
    return acc


def evaluate32_chain(net, images, ns):
    """The float32 yardstick: the forward in the documented operation order (convolution: bias, then (c_in, ky, kx) ascending; Linear and
    RNN: b_ih + b_hh in float32, then W_ih over k ascending, then W_hh over k ascending; tanh = tanh_formula32), every step rounded to
    float32, multiply and add separately.  A numpy loop over k with vectors over rows and units.  -> (rnn_in, q) float32."""
    f = lambda a: np.asarray(a, dtype=np.float32)
    n, T = images.shape[:2]
    x = f(images).reshape(n * T, *images.shape[2:])
    K = net["k"]
    for (co, s, p, d), W, b in zip(net["convs"], net["cw"], net["cb"]):
        W, b = f(W), f(b)
        Hi = x.shape[-1]
        Ho = (Hi + 2 * p - d * (K - 1) - 1) // s + 1
        xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
        acc = np.zeros((x.shape[0], co, Ho, Ho), dtype=np.float32) + b[None, :, None, None]
        for ci in range(x.shape[1]):
            for ky in range(K):
                for kx in range(K):
                    patch = xp[:, ci, ky * d:ky * d + s * (Ho - 1) + 1:s, kx * d:kx * d + s * (Ho - 1) + 1:s]
                    acc = acc + patch[:, None] * W[None, :, ci, ky, kx, None, None]
        assert acc.dtype == np.float32
        x = np.where(acc <= 0, np.float32(0.0), acc)
    rnn_in = np.concatenate([x.reshape(n, T, -1), f(ns)], axis=2)
    H, L = net["H"], net["L"]
    h = [None] * L
    for t in range(T):
        below = rnn_in[:, t]
        for l in range(L):
            acc = np.zeros((n, H), dtype=np.float32) + (f(net["b_ih"][l]) + f(net["b_hh"][l]))[None, :]
            acc = chain32(acc, net["w_ih"][l], below)
            if t > 0:
                acc = chain32(acc, net["w_hh"][l], h[l])
            h[l] = tanh_formula32(acc)
            below = h[l]
    z = h[-1]
    for l, (W, b) in enumerate(zip(net["hw"], net["hb"])):
        z = chain32(np.zeros((n, W.shape[0]), dtype=np.float32) + f(b)[None, :], W, z)
        if l < len(net["hw"]) - 1:
            z = np.where(z > 0, z, np.float32(net["slopes"][l]) * z)
        assert z.dtype == np.float32
    return rnn_in, z


# ---- the tanh grid and the ulp measure -----------------------------------------------------------------------------------------------------
def tanh_grid():
    """Finite float32 arguments, both signs of each: per exponent 2^-126 .. 2^4 512 mantissas (256 evenly spaced, 256 random, fixed seed);
    the float32 neighbours of 16 and 16 itself; 9.0 .. 9.1 densely; 1e30, FLT_MAX; a block of subnormals.  A multiple of 32 values, symmetric."""
    rng = np.random.default_rng(20240)
    man = np.concatenate([np.arange(256, dtype=np.uint32) << 15, rng.integers(0, 1 << 23, size=256, dtype=np.uint32)])
    pos = [((np.uint32(e + 127) << 23) | man).view(np.float32) for e in range(-126, 5)]
    sixteen = np.float32(16.0)
    pos.append(np.array([np.nextafter(sixteen, np.float32(0)), sixteen, np.nextafter(sixteen, np.float32(32)), 1e30, np.finfo(np.float32).max], dtype=np.float32))
    pos.append(np.arange(np.float32(9.0).view(np.uint32), np.float32(9.1).view(np.uint32), 64, dtype=np.uint32).view(np.float32))
    pos.append(np.concatenate([np.arange(1, 257, dtype=np.uint32), rng.integers(1, 1 << 23, size=255, dtype=np.uint32), [np.uint32((1 << 23) - 1)]]).astype(np.uint32).view(np.float32))
    pos = np.unique(np.concatenate(pos))
    grid = np.concatenate([pos, -pos])
    fill = (-len(grid)) % 32  # (even, as the grid is: whole rows of 32 are made up with +-0.5)
    return np.concatenate([grid, np.tile(np.array([0.5, -0.5], dtype=np.float32), fill // 2)]).astype(np.float32)


FLT_MIN = float(np.finfo(np.float32).tiny)  # 2^-126


def ulp_error(got, x):
    """|got - tanh(x)| against float64 np.tanh in ulps of the float32 result: the spacing of float32 in the binade of the float64 value
    (2^-24 just below 1, not the 2^-23 of 1.0 itself)."""
    want = np.tanh(x.astype(np.float64))
    _, e = np.frexp(np.abs(want))
    return np.abs(got.astype(np.float64) - want) / np.ldexp(1.0, np.maximum(e, -125) - 24)


def worst_ulp(got, x):
    """(maximum ulp error over the arguments of normal magnitude, the argument where it occurs)."""
    normal = np.abs(x) >= np.float32(FLT_MIN)
    err = np.where(normal, ulp_error(got, x), 0.0)
    at = int(np.argmax(err))
    return float(err[at]), float(x[at])


# ---- DESIGN.md's dispatch and LDS rules, restated ------------------------------------------------------------------------------------------
def dispatch(convs, k):
    """((CB, K), per-layer form): CB is the smallest of 4 / 8 / 16 / 32 that holds the stack's widest layer; a layer of at most CB / 2
    channels runs the narrow form where CB > 4."""
    widest = max(co for co, *_ in convs)
    CB = next(cb for cb in (4, 8, 16, 32) if widest <= cb)
    return (CB, k), ["narrow" if CB > 4 and co <= CB // 2 else "full" for co, *_ in convs]


def lds_per_image(N, C, k, convs):
    """Bytes of one image's two activation buffers: buffer 0 holds the input and what layers 1 and 3 write, buffer 1 what layers 0 and 2
    write; the last layer writes global memory."""
    slots, size = [C * N * N, 0], N
    for l, (co, s, p, d) in enumerate(convs[:-1]):
        size = (size + 2 * p - d * (k - 1) - 1) // s + 1
        slots[1 - (l & 1)] = max(slots[1 - (l & 1)], co * size * size)
    return 4 * sum(slots)


def rnn_lds(L, dims):
    """Bytes of the recurrence's L + 1 hidden-state buffers: 64 rows x the widest of the hidden size and the head's hidden layers."""
    return 4 * (L + 1) * 64 * max(dims[:-1])


LDS_BUDGET = 160 * 1024

# ---- the stacks of test_gpu_spatial_limits.py: (N, C, k, [(out, stride, padding, dilation)], Fn) ---------------------------------------------
LIMIT_STACKS = {
    "cb4_k1": (4, 3, 1, [(4, 1, 0, 1), (3, 2, 1, 1)], 2),
    "cb4_k3": (5, 2, 3, [(3, 1, 1, 1), (4, 1, 0, 2)], 1),
    "cb4_k5": (6, 3, 5, [(4, 1, 2, 1), (2, 2, 4, 2)], 0),
    "cb16_k1": (4, 5, 1, [(16, 1, 0, 1), (8, 1, 0, 1), (9, 3, 1, 1)], 3),
    "cb16_k5": (7, 4, 5, [(13, 1, 2, 1), (8, 2, 2, 1), (16, 1, 4, 2)], 2),
    "cb32_k1": (3, 32, 1, [(32, 1, 0, 1), (16, 1, 1, 1), (17, 4, 0, 1)], 5),  # (see CONSTANT_OUTPUT)
    "cb32_k1_seen": (3, 32, 1, [(32, 1, 0, 1), (16, 1, 1, 1), (17, 2, 0, 1)], 5),
    "cb32_k5": (6, 9, 5, [(32, 1, 2, 1), (16, 1, 2, 1), (25, 3, 3, 2)], 1),
    "cb8_k5_narrow": (5, 2, 5, [(8, 1, 2, 1), (4, 1, 2, 1)], 1),
    "pad8_dil4_k5": (2, 2, 5, [(3, 1, 8, 4), (5, 4, 8, 4)], 1),  # every tap of most pixels is padding
    # what the table above leaves of the twelve compiled forms and their narrow layers
    "cb8_k1_narrow": (4, 3, 1, [(7, 1, 0, 1), (4, 2, 1, 1)], 2),
    "cb8_k3_narrow": (5, 3, 3, [(4, 1, 1, 1), (8, 2, 1, 1)], 1),
    "cb16_k3_narrow": (6, 4, 3, [(16, 1, 1, 1), (8, 1, 0, 1), (11, 2, 1, 2)], 2),
    "cb32_k3_narrow": (4, 6, 3, [(16, 1, 1, 1), (32, 2, 1, 1)], 3),
}
# the last layer of "cb32_k1" samples its 5 x 5 input at stride 4 -- the four corners, all of them layer 1's padding ring, where a 1 x 1
# kernel gives ReLU(bias): the stack runs <32, 1> and its narrow layer, but its answer does not depend on the image.  "cb32_k1_seen" is
# the same stack at stride 2, whose centre pixel does.
CONSTANT_OUTPUT = {"cb32_k1"}
LDS_STACKS = {
    "lds_over_48k": (16, 32, 3, [(32, 1, 1, 1), (4, 4, 0, 1)], 0),  # 64 KiB per image: one image per group, the opt-in branch
    "lds_160k": (16, 32, 1, [(32, 1, 8, 1), (32, 4, 0, 1)], 0),  # 32 KiB + 128 KiB: exactly the budget, R = 2048
}
R4096_STACK = (16, 1, 3, [(16, 1, 1, 1)], 0)
NINE_BY_NINE = (9, 7, 3, [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)], 8)  # test_gpu_spatial.py's whole-network stack
EXACT_SLOPES = [-2.0, 0.25, 0.0, 4.0, -0.5, 1.0]  # distinct, signed powers of two and 0: a negative one, a zero, one above 1
REAL_SLOPES = [-0.3, 1.7, 0.25, 0.6, 0.05, 1.2]  # distinct reals: a negative one and one above 1
# the whole-network exact cases at the limits: name -> (stack, T, L, H, head, slopes or None for 0.5, n values)
HEAD7 = [128, 64, 32, 16, 8, 4, 6]
WHOLE_LIMITS = {
    "r4096_h256_t8_out32": (R4096_STACK, 8, 1, 256, [256, 32], None, (70,)),  # R, H and the outputs at their limits
    "l4_h128_t8_head7": (NINE_BY_NINE, 8, 4, 128, HEAD7, EXACT_SLOPES, (1, 70, 130)),  # the recurrence's LDS exactly at the budget
    "l2_h213": (NINE_BY_NINE, 3, 2, 213, [6], None, (70,)),  # the widest H at L = 2: neither a multiple of 32 nor even
    "slopes_head3_h33": (NINE_BY_NINE, 2, 1, 33, [16, 9, 5], [-0.5, 4.0], (70,)),
    "slopes_head7_h33": (NINE_BY_NINE, 2, 1, 33, [33, 17, 31, 9, 12, 7, 5], EXACT_SLOPES, (70,)),
}
# name: (stack, L, H, T, head, n values, scale overrides, whether some pre-activation must pass 16)
REAL_CASES = {
    "a_cb32_k5_l4_h128_t8": (LIMIT_STACKS["cb32_k5"], 4, 128, 8, [128, 64, 32], (70,), {}, False),
    "b_r4096_l1_h256_t4": (R4096_STACK, 1, 256, 4, [256, 48, 32], (70,), {}, False),
    "c_cb16_k1_l2_h33_t3_head7": (LIMIT_STACKS["cb16_k1"], 2, 33, 3, [31, 17, 33, 8, 5, 9, 6], (70, 1), dict(w_ih0=2.5, w_ih=2.5), False),
    "d_cb4_k3_l3_h64_t8": (LIMIT_STACKS["cb4_k3"], 3, 64, 8, [16, 12, 6], (70,), {}, False),
    "d_cb4_k3_l3_h64_t8_past16": (LIMIT_STACKS["cb4_k3"], 3, 64, 8, [16, 12, 6], (70,), dict(w_ih0=9.0), True),
}


def real_case(name, n):
    """The network and float32-representable inputs (float64 arrays) of a REAL_CASES entry at n rows: (net, images, ns)."""
    (N, Cc, k, convs, Fn), L, H, T, head, _, scales, _ = REAL_CASES[name]
    rng = np.random.default_rng(sorted(REAL_CASES).index(name) * 1000 + n)
    net = make_net(rng, N, Cc, k, convs, Fn, L, H, head, slopes=REAL_SLOPES[:len(head) - 1], real=True, scales=scales)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    images = f32(np.abs(rng.standard_normal((n, T, Cc, N, N))) * (rng.random((n, T, Cc, N, N)) < 0.6))
    ns = f32(rng.standard_normal((n, T, Fn)))
    return net, images, ns


def regime_fractions(pre):
    """The shares of RNN pre-activations with |z| < 0.25, 0.25 <= |z| <= 2 and |z| > 2, and max |z|."""
    a = np.abs(pre)
    return float((a < 0.25).mean()), float(((a >= 0.25) & (a <= 2.0)).mean()), float((a > 2.0).mean()), float(a.max())


def assert_regimes(ref, past16, n):
    """A real-valued case is not degenerate: each of the three ranges of |z| holds at least 5 % of the RNN's pre-activations, some |z|
    passes 16 where the case is meant to reach tanh's switch, and the float64 Q rows are not all equal."""
    small, middle, large, top = regime_fractions(ref["pre"])
    assert min(small, middle, large) >= 0.05, (small, middle, large)
    assert top > 16.0 or not past16, top
    assert n == 1 or len(np.unique(ref["q"], axis=0)) > n // 2


def stack_seed(name):
    return zlib.crc32(name.encode()) % 100000


def slope_swap_changes(net, inp, l):
    """Whether the float64 answer changes when head layer l takes layer 0's slope."""
    swapped = list(net["slopes"])
    swapped[l] = swapped[0]
    base = evaluate64(net, inp["rows_x"], inp["rows_ns"], check=False)["q"]
    return bool((evaluate64(net, inp["rows_x"], inp["rows_ns"], slopes=swapped, check=False)["q"] != base).any())


# ---- through the C ABI -------------------------------------------------------------------------------------------------------------------
def to_device_at_odd_offsets(arrays):
    """Every array inside ONE float32 allocation at a 4-byte offset that is no multiple of 8 or 16 bytes more often than not."""
    total = sum(a.size + 1 for a in arrays) + 1
    flat = torch.full((total,), CANARY, dtype=torch.float32, device=DEV)
    views, off = [], 1
    for a in arrays:
        v = flat[off:off + a.size].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        views.append(v)
        off += a.size + 1
    return flat, views


def padded(shape, pad):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.float32, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


def spatial_forward(pkg, env, net, dev, spatial, sp_strides, non_spatial, ns_strides, agents, n, T, rnn_in, q_out):
    """susnet_spatial_forward by hand; ``dev``: the network's device tensors as make_net orders them."""
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
    with torch.cuda.device(env.device):
        L.check(env.lib.susnet_spatial_forward(env._h, C.byref(io), env._stream()))


def upload(net):
    keys = ("cw", "cb", "w_ih", "w_hh", "b_ih", "b_hh", "hw", "hb")
    arrays = [a for k in keys for a in net[k]] + [np.full(1, s) for s in net["slopes"]]
    flat, views = to_device_at_odd_offsets(arrays)
    dev, at = {"flat": flat}, 0
    for k in keys:
        dev[k] = views[at:at + len(net[k])]
        at += len(net[k])
    dev["slope"] = views[at:]
    return dev


# agents per env for n rows: 3 where 3 divides n (33), else 5 (95, 320), and 1 for the single row -- there the shared pattern's agent
# stride of 0 has nothing to share, so the stride-0 sharing is exercised at n = 33, 95 and 320 only
def agents_of(n):
    return next(a for a in (3, 5, 1) if n % a == 0)


def exact_inputs(net, n, T, pattern, rng):
    """The integer-valued inputs of one call on `n` rows in one of the stride patterns ("shared": one image per env, "persp": per-agent
    images and non-spatial rows, "shared_ns": per-agent images and ONE non-spatial row per env, agent stride 0): the arrays as they lie in
    memory with their shapes and strides, and the same per row."""
    A = agents_of(n)
    B = n // A
    Cc, N, Fn = net["C"], net["N"], net["Fn"]
    img = lambda *lead: rng.choice([0.0, 1.0, 2.0, 3.0], size=(*lead, Cc, N, N), p=[0.7, 0.2, 0.07, 0.03])
    if pattern == "shared_ns":
        ns = rng.choice([0.0, 1.0, 2.0, 3.0], size=(B, T, Fn), p=[0.6, 0.3, 0.07, 0.03])
    else:
        ns = rng.choice([0.0, 1.0, 2.0, 3.0], size=(B, T, A, Fn), p=[0.6, 0.3, 0.07, 0.03])
    if net["variant"] == "carry":
        ns[:, 1:] = 0.0
    if pattern == "shared":  # the Global featurizer's planes [B][T][C][N][N], agent stride 0
        x = img(B, T)
        rows_x = np.repeat(x[:, None], A, axis=1).reshape(n, T, Cc, N, N)
        sp_strides = (T * Cc * N * N, 0, Cc * N * N)
        sp_shape = (B, T, Cc, N, N)
    else:  # the Perspective featurizer's [B][T][A][C][N][N]
        x = img(B, T, A)
        rows_x = x.transpose(0, 2, 1, 3, 4, 5).reshape(n, T, Cc, N, N)
        sp_strides = (T * A * Cc * N * N, Cc * N * N, A * Cc * N * N)
        sp_shape = (B, T, A, Cc, N, N)
    F1 = max(Fn, 1)
    if pattern == "shared_ns":
        rows_ns = np.repeat(ns[:, None], A, axis=1).reshape(n, T, Fn)
        ns_shape, ns_strides = (B, T, F1), (T * F1, 0, F1)
    else:
        rows_ns = ns.transpose(0, 2, 1, 3).reshape(n, T, Fn)
        ns_shape, ns_strides = (B, T, A, F1), (T * A * F1, F1, A * F1)
    return dict(A=A, x=x, ns=ns, rows_x=rows_x, rows_ns=rows_ns, sp_shape=sp_shape, sp_strides=sp_strides, ns_shape=ns_shape, ns_strides=ns_strides)


def run_exact(pkg, env, net, dev, n, T, pattern, rng):
    """One call on `n` rows in one of exact_inputs' stride patterns; rnn_in and q_out bit-equal to the float64 evaluation, canaries whole,
    inputs unchanged."""
    Fn = net["Fn"]
    inp = exact_inputs(net, n, T, pattern, rng)
    A, x, ns, rows_x, rows_ns, sp_shape, sp_strides, ns_shape, ns_strides = (inp[key] for key in (
        "A", "x", "ns", "rows_x", "rows_ns", "sp_shape", "sp_strides", "ns_shape", "ns_strides"))
    want_in, want_q = evaluate64(net, rows_x, rows_ns)
    sp_buf, sp = padded(sp_shape, 3)
    sp.copy_(torch.from_numpy(x.astype(np.float32)))
    ns_buf, nsd = padded(ns_shape, 5)
    if Fn:
        nsd.copy_(torch.from_numpy(ns.astype(np.float32)))
    in_buf, rnn_in = padded((n, T, net["R"]), 7)
    q_buf, q = padded((n, net["dims"][-1]), 5)
    before = (sp_buf.clone(), ns_buf.clone(), dev["flat"].clone())
    spatial_forward(pkg, env, net, dev, sp, sp_strides, nsd, ns_strides, A, n, T, rnn_in, q)
    torch.cuda.synchronize()
    what = (net["convs"], net["H"], net["L"], n, T, pattern)
    got_in, got_q = rnn_in.cpu().numpy(), q.cpu().numpy()
    assert np.array_equal(got_in.view(np.int32), want_in.view(np.int32)), (what, "rnn_in", float(np.abs(got_in - want_in).max()))
    assert np.array_equal(got_q.view(np.int32), want_q.view(np.int32)), (what, "q_out", float(np.abs(got_q - want_q).max()))
    for buf, pad in ((in_buf, 7), (q_buf, 5)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), (what, "canary")
    assert torch.equal(before[0], sp_buf) and torch.equal(before[1], ns_buf) and torch.equal(before[2], dev["flat"]), (what, "inputs changed")
    return want_q


def forward_rows(pkg, env, net, dev, rows_x, rows_ns):
    """One call on rows given as they are -- rows_x [n, T, C, N, N], rows_ns [n, T, Fn], one agent per env -- between canaries;
    -> (rnn_in [n, T, R], q [n, n_out]) as numpy float32."""
    n, T = rows_x.shape[:2]
    Cc, N, Fn = net["C"], net["N"], net["Fn"]
    F1 = max(Fn, 1)
    sp_buf, sp = padded((n, T, Cc, N, N), 3)
    sp.copy_(torch.from_numpy(np.ascontiguousarray(rows_x, dtype=np.float32)))
    ns_buf, nsd = padded((n, T, F1), 5)
    if Fn:
        nsd.copy_(torch.from_numpy(np.ascontiguousarray(rows_ns, dtype=np.float32)))
    in_buf, rnn_in = padded((n, T, net["R"]), 7)
    q_buf, q = padded((n, net["dims"][-1]), 5)
    spatial_forward(pkg, env, net, dev, sp, (T * Cc * N * N, 0, Cc * N * N), nsd, (T * F1, 0, F1), 1, n, T, rnn_in, q)
    torch.cuda.synchronize()
    for buf, pad in ((in_buf, 7), (q_buf, 5)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), "canary"
    return rnn_in.cpu().numpy(), q.cpu().numpy()
