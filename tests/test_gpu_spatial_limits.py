"""The SpatialDQN forward kernels (susnet_spatial_forward) where tests/test_gpu_spatial.py does not reach: every compiled (CB, K) form of
the convolution kernel and its narrow layers, the LDS opt-in launch and both kernels exactly at the 160 KiB budget, R / H / T / the head /
the outputs at their limits, distinct PReLU slopes, the third stride pattern -- all bit-exact on integer-valued networks -- then tanh
measured through the kernel on a grid of 138 000 arguments, real-valued networks against float64 with a float32 yardstick, row isolation
under non-finite inputs, and the wrapper's paths (Fn = 0, shared non-spatial rows, sliced inputs, a caller's output, changing shapes)
against the torch module.  The networks, references and tables are tests/spatial_exact.py; test_spatial_exact_host.py checks them on the
CPU.  DESIGN.md ("The SpatialDQN forward kernels", Accuracy) records the figures printed here."""
import importlib

import numpy as np
import pytest
import torch

import spatial_exact as X
from spatial_exact import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def handle(pkg):
    env = pkg.BatchedFourRoomEnv(1, 3, 5, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9, obs=pkg.ObsConfig("flat", ["onehot_pos"]))
    env.reset()
    return env


def tol(want):
    return 2e-5 * float(want.abs().max())  # the project's Q-network tolerance (test_gpu_mlp_dense.py)


# ---- 1. every compiled form, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", list(X.LIMIT_STACKS))
def test_every_compiled_convolution_form_is_exact(pkg, handle, stack):
    N, Cc, k, convs, Fn = X.LIMIT_STACKS[stack]
    rng = np.random.default_rng(X.stack_seed(stack))
    net = X.make_net(rng, N, Cc, k, convs, Fn, L=1, H=16, head=[3])
    dev = X.upload(net)
    for n in (1, 95):
        for T in (1, 2):
            for pattern in ("shared", "persp"):
                X.run_exact(pkg, handle, net, dev, n, T, pattern, rng)


# ---- 2. the LDS edges and the limits, exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", list(X.LDS_STACKS))
def test_convolution_is_exact_above_the_grouping_target_and_at_the_lds_budget(pkg, handle, stack):
    """64 KiB per image: one image per group and the LDS opt-in; 160 KiB: the served maximum, launched."""
    N, Cc, k, convs, Fn = X.LDS_STACKS[stack]
    assert X.lds_per_image(N, Cc, k, convs) > 48 * 1024
    rng = np.random.default_rng(X.stack_seed(stack))
    net = X.make_net(rng, N, Cc, k, convs, Fn, L=1, H=16, head=[3])
    dev = X.upload(net)
    for n in (1, 35):
        X.run_exact(pkg, handle, net, dev, n, 2, "persp" if n % 2 else "shared", rng)


def whole_limit(name):
    stack, T, L, H, head, slopes, ns = X.WHOLE_LIMITS[name]
    rng = np.random.default_rng(X.stack_seed(name))
    return X.make_net(rng, *stack, L, H, head, slopes=slopes), T, ns, rng


@pytest.mark.parametrize("case", ["r4096_h256_t8_out32", "l4_h128_t8_head7", "l2_h213"])
def test_whole_network_is_exact_at_the_limits(pkg, handle, case):
    """R = 4096 with H = 256, T = 8 and 32 outputs; the recurrence's LDS exactly at the budget (L = 4, H = 128) under a 7-layer head with
    six distinct slopes; the widest H at L = 2."""
    net, T, ns, rng = whole_limit(case)
    assert X.rnn_lds(net["L"], net["dims"]) <= X.LDS_BUDGET
    dev = X.upload(net)
    for n in ns:
        want = X.run_exact(pkg, handle, net, dev, n, T, "persp", rng)
    assert len(np.unique(want, axis=0)) > 3, "the rows differ: the answer depends on the input"


@pytest.mark.parametrize("case", ["slopes_head3_h33", "slopes_head7_h33"])
def test_every_head_layer_uses_its_own_slope(pkg, handle, case):
    """Distinct slopes -- negative, zero, above 1 -- and a float64 answer that changes when any layer l > 0 takes layer 0's slope."""
    net, T, ns, rng = whole_limit(case)
    assert len(set(net["slopes"])) == len(net["slopes"])
    probe = X.exact_inputs(net, 33, T, "persp", np.random.default_rng(1))
    assert all(X.slope_swap_changes(net, probe, l) for l in range(1, len(net["slopes"]))), "the case can see a slope taken from the wrong layer"
    dev = X.upload(net)
    for n in ns:
        X.run_exact(pkg, handle, net, dev, n, T, "shared", rng)
        X.run_exact(pkg, handle, net, dev, n, T, "persp", rng)


@pytest.mark.parametrize("stack", ["cb16_k1", "cb32_k1_seen", "nine_by_nine"])
def test_non_spatial_rows_shared_by_all_agents(pkg, handle, stack):
    """Non-spatial [B, T, Fn] with an agent stride of 0 under per-agent images: the pattern SpatialQNet.forward advertises."""
    N, Cc, k, convs, Fn = X.NINE_BY_NINE if stack == "nine_by_nine" else X.LIMIT_STACKS[stack]
    assert Fn > 0
    rng = np.random.default_rng(X.stack_seed(stack) + 1)
    net = X.make_net(rng, N, Cc, k, convs, Fn, L=2, H=33, head=[7, 5], slopes=[-0.5])
    dev = X.upload(net)
    for n in (33, 95):
        want = X.run_exact(pkg, handle, net, dev, n, 2, "shared_ns", rng)
    assert len(np.unique(want, axis=0)) > 3


# ---- 3. tanh, measured through the kernel --------------------------------------------------------------------------------------------------
def identity_net():
    """q_out[s][j] = the kernel's tanh of non_spatial[s][0][j]: one zero convolution channel, w_ih = [0 | I], biases 0, a head of I."""
    net = X.make_net(np.random.default_rng(0), 1, 1, 1, [(1, 1, 0, 1)], 32, L=1, H=32, head=[32])
    assert net["R"] == 33 and net["dims"] == [32, 32]
    net["cw"][0][:], net["cb"][0][:] = 0.0, 0.0
    net["w_ih"][0] = np.concatenate([np.zeros((32, 1)), np.eye(32)], axis=1)
    net["w_hh"][0][:], net["b_ih"][0][:], net["b_hh"][0][:] = 0.0, 0.0, 0.0
    net["hw"][0], net["hb"][0] = np.eye(32), np.zeros(32)
    return net


def test_tanh_through_the_kernel(pkg, handle):
    """Measured on the MI355X: DESIGN.md ("The SpatialDQN forward kernels", Accuracy) records the figures this test prints."""
    x = X.tanh_grid()
    rows = x.reshape(-1, 1, 32)
    net = identity_net()
    rnn_in, q = X.forward_rows(pkg, handle, net, X.upload(net), np.zeros((len(rows), 1, 1, 1, 1)), rows)
    assert np.array_equal(rnn_in[:, 0, 1:].view(np.int32), rows[:, 0].view(np.int32)) and not rnn_in[:, 0, 0].any()
    t = q.reshape(-1)
    ax, at = np.abs(x), np.abs(t)
    order = np.argsort(x, kind="stable")
    xs, ts = x[order], t[order]
    # (a) odd: t(-x) is -t(x) bit for bit (a zero's sign apart: the head adds 31 products that are +0)
    pos, neg = x > 0, x < 0
    up = dict(zip(x[pos].view(np.int32).tolist(), t[pos].tolist()))
    down = dict(zip((-x[neg]).view(np.int32).tolist(), t[neg].tolist()))
    assert up.keys() == down.keys()
    odd = [key for key in up if not (up[key] == -down[key])]
    assert not odd, (len(odd), np.array(odd[:5], dtype=np.int32).view(np.float32))
    # (b) range
    assert (at <= 1.0).all() and (at[ax >= 16.0] == 1.0).all() and (np.sign(t)[at > 0] == np.sign(x)[at > 0]).all()
    # the formula's own error on this grid (an accurate expm1), and the cap it gives
    formula, formula_at = X.worst_ulp(X.tanh_formula32(x), x)
    cap = formula + 2.0  # expm1f's permitted 1 ulp (ROCm's HIP math table), amplified by at most 2 where e -> -1: d/de[-e / (e + 2)] = -2 / (e + 2)^2
    worst, worst_at = X.worst_ulp(t, x)
    with torch.no_grad():
        torch_t = torch.tanh(torch.from_numpy(x).to(DEV)).cpu().numpy()
    torch_worst, torch_at = X.worst_ulp(torch_t, x)
    sub = ax < np.float32(X.FLT_MIN)
    flushed = int((t[sub] == 0).sum())
    print(f"tanh on {len(x)} arguments: kernel max {worst:.3f} ulp at x = {worst_at!r}; formula with an accurate expm1 {formula:.3f} ulp at x = {formula_at!r} "
          f"(cap {cap:.3f}); torch.tanh on the device {torch_worst:.3f} ulp at x = {torch_at!r}; subnormal arguments answered with 0: {flushed} of {int(sub.sum())}")
    # (c) monotone non-decreasing over the sorted grid, up to the cap
    ulp = np.ldexp(1.0, np.maximum(np.frexp(np.maximum(np.abs(ts), np.float32(X.FLT_MIN)).astype(np.float64))[1], -125) - 24)
    running = np.maximum.accumulate(ts.astype(np.float64))
    drop = (running - ts.astype(np.float64)) / ulp
    assert float(drop.max()) <= cap, (float(drop.max()), float(xs[int(np.argmax(drop))]))
    # (d) accuracy on arguments of normal magnitude
    assert worst <= cap, f"sp_tanh: {worst:.3f} ulp at x = {worst_at!r} against float64 tanh; the cap is {cap:.3f} (formula {formula:.3f} + 2)"
    # (e) subnormal arguments: tanh x = x to far below an ulp; a flush to zero is tolerated (and reported above)
    assert (np.abs(t[sub].astype(np.float64) - x[sub].astype(np.float64)) <= X.FLT_MIN).all()


# ---- 4. real-valued networks against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(X.REAL_CASES))
def test_real_valued_networks_against_float64(pkg, handle, case):
    """max |kernel - float64| over q_out and over rnn_in, against the same for the float32 yardstick (evaluate32_chain: the documented
    operation order and tanh formula, no fused multiply-add): the kernel's error is at most twice the yardstick's.  DESIGN.md records the
    measured ratios."""
    stack, L, H, T, head, ns_, scales, past16 = X.REAL_CASES[case]
    for n in ns_:
        net, images, ns = X.real_case(case, n)
        ref = X.evaluate64(net, images, ns)
        X.assert_regimes(ref, past16, n)
        yard_in, yard_q = X.evaluate32_chain(net, images, ns)
        got_in, got_q = X.forward_rows(pkg, handle, net, X.upload(net), images, ns)
        cols = net["conv_cols"]
        assert np.array_equal(got_in[:, :, cols:].view(np.int32), ns.astype(np.float32).view(np.int32)), "the non-spatial columns are copies"
        err = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())
        k_q, y_q, k_in, y_in = err(got_q, ref["q"]), err(yard_q, ref["q"]), err(got_in, ref["rnn_in"]), err(yard_in, ref["rnn_in"])
        print(f"{case} n={n}: max|q| {float(np.abs(ref['q']).max()):.3f}; q_out kernel {k_q:.3e} yardstick {y_q:.3e} ratio {k_q / y_q:.2f}; "
              f"rnn_in kernel {k_in:.3e} yardstick {y_in:.3e} ratio {k_in / y_in:.2f}")
        assert y_q > 0 and y_in > 0
        assert k_in <= 2.0 * y_in, f"{case} n={n}: rnn_in: kernel {k_in:.3e} > 2 x yardstick {y_in:.3e}"
        assert k_q <= 2.0 * y_q, f"{case} n={n}: q_out: kernel {k_q:.3e} > 2 x yardstick {y_q:.3e}"


# ---- 5. row isolation ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_leave_the_other_rows_untouched(pkg, handle):
    """Rows 5, 64 and the last carry +Inf, -Inf, NaN and 3e38 in their images and non-spatial rows; every other row of their 64-row tiles
    and 16-image groups answers bit for bit as without them."""
    n, T = 130, 3
    rng = np.random.default_rng(55)
    net = X.make_net(rng, *X.NINE_BY_NINE, 3, 33, [7])  # test_gpu_spatial.py's t3_l3_h33
    dev = X.upload(net)
    inp = X.exact_inputs(net, n, T, "persp", rng)
    rows_x, rows_ns = inp["rows_x"].astype(np.float32), inp["rows_ns"].astype(np.float32)
    clean_in, clean_q = X.forward_rows(pkg, handle, net, dev, rows_x, rows_ns)
    want_in, want_q = X.evaluate64(net, inp["rows_x"], inp["rows_ns"])
    assert np.array_equal(clean_in.view(np.int32), want_in.view(np.int32)) and np.array_equal(clean_q.view(np.int32), want_q.view(np.int32))
    bad = np.array([5, 64, n - 1])
    poison = np.array([np.inf, -np.inf, np.nan, 3e38], dtype=np.float32)
    dirty_x, dirty_ns = rows_x.copy(), rows_ns.copy()
    dirty_x[bad] = rng.choice(poison, size=dirty_x[bad].shape)
    dirty_ns[bad] = rng.choice(poison, size=dirty_ns[bad].shape)
    got_in, got_q = X.forward_rows(pkg, handle, net, dev, dirty_x, dirty_ns)
    others = np.setdiff1d(np.arange(n), bad)
    assert np.array_equal(got_in[others].view(np.int32), clean_in[others].view(np.int32)), "rnn_in of the other rows"
    assert np.array_equal(got_q[others].view(np.int32), clean_q[others].view(np.int32)), "q_out of the other rows"
    assert not np.isfinite(got_in[bad]).all()  # (the poisoned rows did go through the kernels)


# ---- 6. the wrapper's paths, against the torch module ----------------------------------------------------------------------------------------
def seeded_module(pkg, Fn, seed=11, **over):
    cfg = dict(input_image_size=9, non_spatial_input_size=Fn, n_channels=[5, 6, 8], strides=[1, 1], paddings=[1, 1], kernel_size=(3, 3), dilations=[1, 1],
               rnn_layers=2, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[16, 12], n_actions=6)
    cfg.update(over)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = pkg.SpatialDQN(**cfg)
        with torch.no_grad():
            for name, p in m.named_parameters():  # (a default initialisation answers every input nearly alike)
                if p.dim() > 1:
                    p.mul_(3.0)
            m.prediction_head[1].weight.fill_(-0.3)
            m.prediction_head[3].weight.fill_(1.7)
    return m.to(DEV).eval()


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV)


def per_agent(model, spatial, non_spatial, agents):
    """The module called once per agent view; non_spatial [B, T, Fn] is every agent's."""
    with torch.no_grad():
        rows = [model(spatial[:, :, i], non_spatial[:, :, i] if non_spatial.dim() == 4 else non_spatial) for i in range(agents)]
    return torch.stack(rows, dim=1).reshape(-1, rows[0].shape[-1])


def close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= tol(want), f"{what}: max error {err:.3e} > {tol(want):.3e}"
    assert len(torch.unique(want, dim=0)) > 3


def test_wrapper_serves_a_model_without_non_spatial_features(pkg, handle):
    model = seeded_module(pkg, 0)
    net = pkg.SpatialQNet(handle, model)
    assert net is not None and net.Fn == 0
    gen = torch.Generator(device=DEV).manual_seed(1)
    spatial = randn(gen, 37, 3, 5, 9, 9)
    empty = torch.empty(37, 3, 0, device=DEV)
    assert empty.data_ptr() == 0  # (what the call is handed: no storage)
    with torch.no_grad():
        want = model(spatial, empty)
    close(net.forward(spatial, empty), want, "Fn = 0, one agent")
    views = randn(gen, 12, 2, 3, 5, 9, 9)
    close(net.forward(views, torch.empty(12, 2, 3, 0, device=DEV), 3), per_agent(model, views, torch.empty(12, 2, 3, 0, device=DEV), 3), "Fn = 0, agent views")


def test_wrapper_paths_against_the_torch_module(pkg, handle):
    model = seeded_module(pkg, 7)
    net = pkg.SpatialQNet(handle, model)
    gen = torch.Generator(device=DEV).manual_seed(2)
    A = 3
    # non-spatial rows shared by all agents under per-agent images
    spatial, shared = randn(gen, 21, 3, A, 5, 9, 9), randn(gen, 21, 3, 7)
    close(net.forward(spatial, shared, A), per_agent(model, spatial, shared, A), "shared non-spatial")
    # batch slices of larger tensors: the env stride is the parent's, the storage offset is not 0
    big_x, big_ns = randn(gen, 50, 3, A, 5, 9, 9), randn(gen, 50, 3, A, 7)
    x, ns = big_x[3:40], big_ns[3:40]
    assert x.storage_offset() > 0 and ns.storage_offset() > 0
    want = per_agent(model, x, ns, A)
    close(net.forward(x, ns, A), want, "sliced inputs")
    # a caller's output between canaries
    buf, out = X.padded((37 * A, 6), 9)
    got = net.forward(x, ns, A, out=out)
    assert got.data_ptr() == out.data_ptr()
    close(out, want, "out=")
    assert bool((buf[:9] == X.CANARY).all()) and bool((buf[-9:] == X.CANARY).all())
    # another B, then another T, on the same object: the workspace and the default output are re-made
    first = net.forward(x, ns, A)
    kept = first.clone()
    x2, ns2 = randn(gen, 11, 3, A, 5, 9, 9), randn(gen, 11, 3, A, 7)
    second = net.forward(x2, ns2, A)
    assert tuple(second.shape) == (11 * A, 6) and tuple(net._rnn_in.shape) == (11 * A, 3, net.R)
    close(second, per_agent(model, x2, ns2, A), "after B changed")
    x3, ns3 = randn(gen, 11, 5, A, 5, 9, 9), randn(gen, 11, 5, A, 7)
    third = net.forward(x3, ns3, A).clone()
    assert tuple(net._rnn_in.shape) == (11 * A, 5, net.R)
    close(third, per_agent(model, x3, ns3, A), "after T changed")
    close(net.forward(x, ns, A), kept, "back at the first shape")
    assert torch.equal(net.forward(x, ns, A), kept)
