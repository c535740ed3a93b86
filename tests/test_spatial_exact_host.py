"""CPU checks behind the tests of the SpatialDQN forward kernels at their limits (tests/spatial_exact.py, tests/test_gpu_spatial_limits.py):
the GPU test's stack tables reach every compiled form and the LDS edges they are meant to reach, every exact case passes the float64
evaluator's exactness guards, the evaluator agrees with the torch mirror of the reference module, the float32 yardstick agrees with the
evaluator within the float32 error to expect, the documented tanh formula's own error is measured, and the real-valued cases put the RNN's
pre-activations where tanh is a function and not a constant -- conditions on the REFERENCES, met without a GPU."""
import importlib

import numpy as np
import pytest
import torch

import spatial_exact as X


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_the_stack_tables_reach_every_compiled_form_and_each_narrow_layer():
    forms, narrow = set(), set()
    for N, Cc, k, convs, Fn in list(X.LIMIT_STACKS.values()) + list(X.LDS_STACKS.values()):
        form, layers = X.dispatch(convs, k)
        forms.add(form)
        if "narrow" in layers:
            narrow.add(form)
        assert "full" in layers  # (the widest layer itself)
    assert forms == {(cb, k) for cb in (4, 8, 16, 32) for k in (1, 3, 5)}
    assert narrow == {(cb, k) for cb in (8, 16, 32) for k in (1, 3, 5)}  # (CB = 4 has no narrower form)
    # the issue's table, form by form
    want = dict(cb4_k1=(4, 1), cb4_k3=(4, 3), cb4_k5=(4, 5), cb16_k1=(16, 1), cb16_k5=(16, 5), cb32_k1=(32, 1), cb32_k5=(32, 5), cb8_k5_narrow=(8, 5))
    for name, form in want.items():
        assert X.dispatch(X.LIMIT_STACKS[name][3], X.LIMIT_STACKS[name][2])[0] == form, name
    assert X.dispatch([(5, 1, 1, 1), (3, 1, 1, 1)], 3) == ((8, 3), ["full", "narrow"]) and X.dispatch([(4, 1, 1, 1), (2, 1, 1, 1)], 1) == ((4, 1), ["full", "full"])


def test_lds_sizes_of_the_edge_cases():
    over, full = X.LDS_STACKS["lds_over_48k"], X.LDS_STACKS["lds_160k"]
    assert X.lds_per_image(*over[:4]) == 64 * 1024 > 48 * 1024
    assert X.lds_per_image(*full[:4]) == 163840 == X.LDS_BUDGET
    for N, Cc, k, convs, Fn in X.LIMIT_STACKS.values():
        assert X.lds_per_image(N, Cc, k, convs) <= 48 * 1024 // 4  # (these run four or more images to a group)
    stack, T, L, H, head, slopes, ns = X.WHOLE_LIMITS["l4_h128_t8_head7"]
    assert (L, H, len(head)) == (4, 128, 7) and X.rnn_lds(L, [H] + head) == 163840
    stack, T, L, H, head, slopes, ns = X.WHOLE_LIMITS["l2_h213"]
    assert X.rnn_lds(L, [H] + head) <= X.LDS_BUDGET < X.rnn_lds(L, [H + 1] + head) and H % 2 == 1
    stack, T, L, H, head, slopes, ns = X.WHOLE_LIMITS["r4096_h256_t8_out32"]
    net = X.make_net(np.random.default_rng(0), *stack, L, H, head)
    assert (net["R"], H, head[-1], T) == (4096, 256, 32, 8)
    # the 9x9 stack as the 3x3 / padding-1 rule gives it: 7 x 81 in, 5 x 81 and 3 x 81 between
    assert X.lds_per_image(9, 7, 3, [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)]) == 4 * (7 * 81 + 5 * 81)


# ---- the exact cases are exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.LIMIT_STACKS) + list(X.LDS_STACKS))
def test_every_stack_passes_the_exactness_guards(name):
    """What test_gpu_spatial_limits.py compares bit for bit: evaluate64 asserts sum |w||x| + |b| < 2^24 at every layer."""
    lds = name in X.LDS_STACKS
    N, Cc, k, convs, Fn = (X.LDS_STACKS if lds else X.LIMIT_STACKS)[name]
    rng = np.random.default_rng(X.stack_seed(name))
    net = X.make_net(rng, N, Cc, k, convs, Fn, L=1, H=16, head=[3])
    n = 35 if lds else 95
    inp = X.exact_inputs(net, n, 2, "persp", rng)
    want_in, want_q = X.evaluate64(net, inp["rows_x"], inp["rows_ns"])
    conv = want_in[:, :, :net["conv_cols"]].reshape(n, -1)
    assert want_in.shape == (n, 2, net["R"])
    if name in X.CONSTANT_OUTPUT:  # (the issue's stack, kept as given: it runs its kernel forms, but only its sibling shows their arithmetic)
        assert len(np.unique(conv, axis=0)) == 1 and name + "_seen" in X.LIMIT_STACKS
    else:
        assert len(np.unique(conv, axis=0)) > 3, "the convolution's answer depends on the image"


def test_slopes_are_seen_by_the_exact_heads():
    """Distinct signed power-of-two and zero slopes keep the head exact, and the float64 answer changes when layer l > 0 takes layer 0's."""
    assert len(set(X.EXACT_SLOPES)) == 6 and min(X.EXACT_SLOPES) < 0 and 0.0 in X.EXACT_SLOPES and max(X.EXACT_SLOPES) > 1
    for name in ("slopes_head3_h33", "slopes_head7_h33"):
        stack, T, L, H, head, slopes, ns = X.WHOLE_LIMITS[name]
        rng = np.random.default_rng(X.stack_seed(name))
        net = X.make_net(rng, *stack, L, H, head, slopes=slopes)
        inp = X.exact_inputs(net, 33, T, "persp", rng)
        want_in, want_q = X.evaluate64(net, inp["rows_x"], inp["rows_ns"])
        again = X.evaluate64(net, inp["rows_x"], inp["rows_ns"], check=False)["q"]
        assert np.array_equal(again, want_q.astype(np.float64))
        changed = [l for l in range(1, len(slopes)) if X.slope_swap_changes(net, inp, l)]
        assert changed == list(range(1, len(slopes))), (name, changed)
    with pytest.raises(AssertionError):
        X.slope_denominator(1.5)
    assert [X.slope_denominator(s) for s in (-2.0, 0.25, 0.0, 4.0, -0.5, 1.0)] == [1, 4, 1, 1, 2, 1]


# ---- the evaluator against the torch mirror of the reference module ----------------------------------------------------------------------------
# two configurations the module can express (it appends one more convolution of the last width, which must keep the size: k 3 / padding 1,
# k 5 / padding 2): (N, C, k, convs, Fn, L, H, head, T)
TORCH_CONFIGS = {
    "k3_p1": (7, 3, 3, [(6, 2, 1, 1), (4, 1, 1, 1), (4, 1, 1, 1)], 3, 2, 12, [9, 7, 5], 3),
    "k5_p2_fn0": (6, 2, 5, [(5, 1, 2, 1), (3, 1, 2, 1), (3, 1, 2, 1)], 0, 1, 10, [8, 6, 4, 3], 2),
}


def torch_case(name, n=24):
    N, Cc, k, convs, Fn, L, H, head, T = TORCH_CONFIGS[name]
    rng = np.random.default_rng(sorted(TORCH_CONFIGS).index(name) + 40)
    net = X.make_net(rng, N, Cc, k, convs, Fn, L, H, head, slopes=X.REAL_SLOPES[:len(head) - 1], real=True)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return net, f32(rng.standard_normal((n, T, Cc, N, N))), f32(rng.standard_normal((n, T, Fn)))


def module_of(pkg, net):
    convs = net["convs"]
    assert convs[-1] == convs[-2]
    m = pkg.SpatialDQN(input_image_size=net["N"], non_spatial_input_size=net["Fn"], n_channels=[net["C"]] + [c[0] for c in convs[:-1]],
                       strides=[c[1] for c in convs[:-1]], paddings=[c[2] for c in convs[:-1]], kernel_size=(net["k"], net["k"]),
                       dilations=[c[3] for c in convs[:-1]], rnn_layers=net["L"], rnn_hidden_dim=net["H"], rnn_dropout=0.0,
                       mlp_hidden_layer_dims=net["dims"][1:-1], n_actions=net["dims"][-1]).double().eval()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with torch.no_grad():
        for l in range(len(convs)):
            m.cnn.model[2 * l].weight.copy_(t(net["cw"][l]))
            m.cnn.model[2 * l].bias.copy_(t(net["cb"][l]))
        for l in range(net["L"]):
            for key, name in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
                getattr(m.rnn.model, f"{name}_l{l}").copy_(t(net[key][l]))
        for l in range(len(net["hw"])):
            m.prediction_head[2 * l].weight.copy_(t(net["hw"][l]))
            m.prediction_head[2 * l].bias.copy_(t(net["hb"][l]))
        for l, a in enumerate(net["slopes"]):
            m.prediction_head[2 * l + 1].weight.fill_(a)
    return m


@pytest.mark.parametrize("name", list(TORCH_CONFIGS))
def test_evaluate64_agrees_with_the_torch_module_in_float64(pkg, name):
    net, images, ns = torch_case(name)
    assert len(set(net["slopes"])) == len(net["slopes"]) >= 2
    got = X.evaluate64(net, images, ns)
    with torch.no_grad():
        want = module_of(pkg, net)(torch.from_numpy(images), torch.from_numpy(ns)).numpy()
    err = float(np.abs(got["q"] - want).max())
    print(f"{name}: evaluate64 vs the float64 module: max error {err:.3e}, max |q| {float(np.abs(want).max()):.3f}")
    assert err <= 1e-12 * float(np.abs(want).max())
    assert got["pre"].shape == (images.shape[1], net["L"], images.shape[0], net["H"])


@pytest.mark.parametrize("name", list(TORCH_CONFIGS))
def test_the_float32_yardstick_stays_within_the_expected_float32_error(name):
    """The expectation is evaluate64's own (its body states it): the probabilistic rounding model -- independent roundings of at most
    2^-24, so sqrt(K + 1) u (sum |w||x| + |b|) per chain of K products, the operands' variances carried through W^2 and the activations'
    derivatives -- and the allowance is SIGMAS = 6 standard deviations per element.  (The worst-case bound, gamma(K) carried through |W|,
    is above max |q| itself on these nets: it says nothing.)  That the expectation is not vacuous is asserted too."""
    net, images, ns = torch_case(name)
    ref = X.evaluate64(net, images, ns)
    got_in, got_q = X.evaluate32_chain(net, images, ns)
    assert got_in.dtype == np.float32 and got_q.dtype == np.float32
    e_in, e_q = np.abs(got_in - ref["rnn_in"]), np.abs(got_q - ref["q"])
    conv = slice(0, net["conv_cols"])
    print(f"{name}: yardstick vs float64: rnn_in {float(e_in.max()):.3e} (largest sigma {float(ref['rnn_in_sigma'].max()):.3e}), q {float(e_q.max()):.3e} "
          f"(largest sigma {float(ref['q_sigma'].max()):.3e}; largest error / sigma {float((e_q / ref['q_sigma']).max()):.3f}, "
          f"rnn_in {float((e_in[:, :, conv] / ref['rnn_in_sigma'][:, :, conv]).max()):.3f})")
    assert (e_in <= X.SIGMAS * ref["rnn_in_sigma"]).all() and (e_q <= X.SIGMAS * ref["q_sigma"]).all()
    assert X.SIGMAS * float(ref["q_sigma"].max()) < 1e-3 * float(np.abs(ref["q"]).max())  # (three digits below the answer's size)
    assert float(e_q.max()) > 0.0  # (a float32 evaluation, not the float64 one handed back)
    # the non-spatial columns are copies
    assert np.array_equal(got_in[:, :, net["conv_cols"]:], ns.astype(np.float32))


# ---- the tanh formula --------------------------------------------------------------------------------------------------------------------------
def test_tanh_formula_error_on_the_grid():
    """The documented formula with an ACCURATE expm1, against float64 np.tanh: the formula's own error (the division and e + 2 round), on
    which the GPU test builds its cap.  Measured here: 2.244 ulp at x = 4.1983 (e, e + 2 and the division round: at most 1 + 1 + 0.5 ulp
    where e -> -1; an emulation with a float32 expm1 gave 3.17 ulp at |x| ~ 4.09)."""
    x = X.tanh_grid()
    assert x.dtype == np.float32 and len(x) % 32 == 0 and 130_000 < len(x) < 150_000 and np.isfinite(x).all()
    assert np.float32(16.0) in x and np.nextafter(np.float32(16), np.float32(0)) in x and np.finfo(np.float32).max in x
    assert int((np.abs(x) < np.float32(X.FLT_MIN)).sum()) >= 512 and int(((x >= 9.0) & (x <= 9.1)).sum()) > 1000
    for e in range(-126, 5):
        assert int(((x >= np.float32(2.0 ** e)) & (x < np.float32(2.0 ** (e + 1)))).sum()) >= 500, e
    t = X.tanh_formula32(x)
    worst, at = X.worst_ulp(t, x)
    print(f"tanh_formula32 on {len(x)} points: max error {worst:.3f} ulp at x = {at!r}")
    assert 0.5 <= worst <= 4.0  # (float32 cannot do better than 0.5; three roundings after expm1 do not give more than 4)
    assert np.array_equal(X.tanh_formula32(-x).view(np.int32), (-t).view(np.int32))
    assert (np.abs(t) <= 1).all() and (np.abs(t)[np.abs(x) >= 16] == 1).all()
    sub = np.abs(x) < np.float32(X.FLT_MIN)
    assert (np.abs(t[sub].astype(np.float64) - x[sub].astype(np.float64)) <= X.FLT_MIN).all()
    assert np.array_equal(X.tanh_formula32(np.array([0.0, -0.0, 32.0, -96.0], dtype=np.float32)).view(np.int32),
                          np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32).view(np.int32))


# ---- the real-valued cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.REAL_CASES))
def test_real_cases_spread_the_pre_activations_over_the_regimes_of_tanh(name):
    stack, L, H, T, head, ns_, scales, past16 = X.REAL_CASES[name]
    for n in ns_:
        net, images, ns = X.real_case(name, n)
        assert len(set(net["slopes"])) == len(net["slopes"]) and min(net["slopes"]) < 0 and (len(head) < 3 or max(net["slopes"]) > 1)
        ref = X.evaluate64(net, images, ns)
        X.assert_regimes(ref, past16, n)
        print(name, n, "shares of |z| < 0.25, 0.25..2, > 2 and max |z|:", X.regime_fractions(ref["pre"]))
