"""The fused Q-network kernels (susnet_qnet_forward, susnet_qnet_policy_step) on the MI355X against a float64 evaluation, EXACTLY: integer
networks (tests/qnet_exact.py: every float32 summation order gives the float64 result) on directed states of the three compiled-in
layouts -- every position row, tail row and alive combination, ragged batches, padded widths, both PReLU forms, canaries around the Q
rows -- and tie networks that make the in-register argmax decide between equal maxima within and across the two lane halves.  Every
comparison is an equality."""
import importlib

import numpy as np
import pytest
import torch

import qnet_exact as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 12345.0
ACTION_DTYPES = (torch.int64, torch.int32, torch.uint8)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


_ENVS = {}


def forward_env(pkg, layout, B):
    """One handle per (layout, batch) holding the first B directed states; its flat observation is the oracle's rows bit for bit."""
    if (layout, B) not in _ENVS:
        env = X.make_env(pkg, layout, B, device=DEV, auto_reset=True, check_errors=False)
        env.reset()
        X.import_states(env, X.directed_states(layout), B)
        feats = np_(env.observe(pkg.ObsConfig("flat", X.LAYOUTS[layout]["comps"])))
        assert np.array_equal(feats.view(np.int32), X.oracle_rows(layout)[:B].view(np.int32)), (layout, B, "flat observation vs the oracle")
        _ENVS[(layout, B)] = env
    return _ENVS[(layout, B)]


def pack(env, layout, net):
    W, b, slopes = net
    packed = env.qnet_pack(X.LAYOUTS[layout]["comps"], W, b, slopes)
    assert packed is not None, "the compiled-in network family serves this stack"
    return packed


def forward_in_canaries(env, packed, n_out):
    """qnet_forward into a contiguous [B, n_out] view inside a canary-filled buffer: the rows, and both canaries untouched."""
    B, pad = env.batch, 5
    buf = torch.full((B * n_out + 2 * pad,), CANARY, dtype=torch.float32, device=DEV)
    view = buf[pad:pad + B * n_out].view(B, n_out)
    env.qnet_forward(packed, out=view)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), "a store outside the Q rows"
    return np_(view)


# ---- a. forward, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope_index", range(len(X.SLOPE_SETS)), ids=["unit", "unit-ends", "select"])
@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_qnet_forward_is_exact_on_integer_networks(pkg, layout, slope_index):
    rows = X.oracle_rows(layout)
    for dims, net in X.forward_cases(layout, slope_index):
        want, _ = X.reference_q(net, rows)
        packed = pack(forward_env(pkg, layout, X.BATCHES[-1]), layout, net)
        for B in X.BATCHES:
            got = forward_in_canaries(forward_env(pkg, layout, B), packed, dims[-1])
            X.assert_same_values(got, want[:B], (layout, dims, X.SLOPE_SETS[slope_index], B))


# ---- b. the one-kernel tick: Q rows and greedy actions under ties ---------------------------------------------------------------------------
def expected_actions(states, q_imp, crew):
    """[B, A]: the imposter's slot holds numpy's first maximum of its Q row, the crew's slots ``crew`` ([B, A] draws, or [B] argmaxes)."""
    imp = states["imp"].astype(bool)
    crew = np.asarray(crew, dtype=np.int64)
    return np.where(imp, q_imp.argmax(axis=1)[:, None], crew if crew.ndim == 2 else crew[:, None])


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_one_kernel_tick_is_exact_and_takes_the_first_maximum(pkg, layout, which):
    lay = X.LAYOUTS[layout]
    B, A = X.TICK_BATCH, lay["A"]
    states, rows = X.playable_states(layout), X.playable_rows(layout)
    obs = pkg.ObsConfig("flat", lay["comps"])
    env = X.make_env(pkg, layout, B, device=DEV, seed=23, auto_reset=True, check_errors=True, obs=obs)
    twin = X.make_env(pkg, layout, B, device=DEV, seed=23, auto_reset=True, check_errors=True, obs=obs)
    env.reset()
    twin.reset()
    net_i, net_c = X.tie_network(layout, which, lay["n_imp"]), X.tie_network(layout, which, lay["n_crew"])
    want_i, want_c = X.reference_q(net_i, rows)[0], X.reference_q(net_c, rows)[0]
    pk_i, pk_c = pack(env, layout, net_i), pack(env, layout, net_c)
    assert env.supports_qnet_policy_step(pk_i) and env.supports_qnet_policy_step(pk_i, pk_c)

    def fresh():
        for e in (env, twin):
            X.import_states(e, states)
        assert np.array_equal(np_(env.observe(obs)).view(np.int32), rows.view(np.int32))
        return np_(env.sample_actions().to(torch.int64).clone())  # the crew's draws of this tick

    # a random crew: every action dtype, one tick each
    for dt in ACTION_DTYPES:
        sampled = fresh()
        q = torch.full((B, lay["n_imp"]), CANARY, device=DEV)
        out = torch.zeros(B, A, dtype=dt, device=DEV)
        a = env.qnet_policy_step(pk_i, actions_out=out, q_out=q, epsilon=0.0, mask_dead=False)[5]
        X.assert_same_values(np_(q), want_i, (layout, which, "Q rows of the tick"))
        assert np.array_equal(np_(a).astype(np.int64), expected_actions(states, want_i, sampled)), (layout, which, dt)
        a2 = twin.policy_step(twin.qnet_forward(pk_i), None, actions_out=torch.zeros(B, A, dtype=dt, device=DEV))[5]  # two launches
        assert torch.equal(a, a2), (layout, which, dt, "one kernel vs two launches")
    # both teams by their networks: the crew's pass runs after the LDS image swap
    for dt in ACTION_DTYPES[::-1][:2]:
        fresh()
        q = torch.full((B, lay["n_imp"]), CANARY, device=DEV)
        qc = torch.full((B, lay["n_crew"]), CANARY, device=DEV)
        out = torch.zeros(B, A, dtype=dt, device=DEV)
        a = env.qnet_policy_step(pk_i, actions_out=out, q_out=q, epsilon=0.0, mask_dead=False, net_crew=pk_c, q_crew_out=qc)[5]
        X.assert_same_values(np_(q), want_i, (layout, which, "imposter Q rows, both teams"))
        X.assert_same_values(np_(qc), want_c, (layout, which, "crew Q rows, both teams"))
        assert np.array_equal(np_(a).astype(np.int64), expected_actions(states, want_i, want_c.argmax(axis=1))), (layout, which, dt)
        qi2, qc2 = twin.qnet_forward(pk_i).clone(), twin.qnet_forward(pk_c).clone()
        a2 = twin.policy_step(qi2, qc2, actions_out=torch.zeros(B, A, dtype=dt, device=DEV))[5]
        assert torch.equal(a, a2), (layout, which, dt, "one kernel vs two launches, both teams")
    assert int(env.tick) == int(twin.tick) == 5


# ---- c. the network the train step leaves behind --------------------------------------------------------------------------------------------
def test_policy_image_follows_re_pointed_parameters_exactly(pkg):
    """A PolicyRollout's packed image after the module's parameters were re-pointed to other tensors (what the trainer does when it moves
    them into its flat buffer) and ``refresh_weights(force=True)``: the second network's exact rows, through the same device buffer."""
    layout = "onehot3"
    lay = X.LAYOUTS[layout]
    rows, states = X.oracle_rows(layout), X.directed_states(layout)
    env = X.make_env(pkg, layout, len(rows), device=DEV, auto_reset=True, check_errors=False, obs=pkg.ObsConfig("flat", lay["comps"]))
    env.reset()
    X.import_states(env, states)
    dims = [lay["F"], 200, 100, 50, 10, lay["n_imp"]]
    first, second = X.int_network(dims, 901, X.SLOPE_SETS[0]), X.int_network(dims, 902, X.SLOPE_SETS[2])

    def tensors(net):
        W, b, slopes = net
        out = []
        for l in range(5):
            out += [torch.tensor(W[l], dtype=torch.float32, device=DEV), torch.tensor(b[l], dtype=torch.float32, device=DEV)]
            if l < 4:
                out.append(torch.tensor([slopes[l]], dtype=torch.float32, device=DEV))
        return out

    model = pkg.MLP(dims).to(DEV).eval()
    params = list(model.parameters())  # Linear weight, bias, PReLU slope, ... in module order
    assert [tuple(p.shape) for p in params] == [tuple(t.shape) for t in tensors(first)]
    with torch.no_grad():
        for p, t in zip(params, tensors(first)):
            p.copy_(t)
    pol = pkg.PolicyRollout(env, model, None, components=lay["comps"])
    assert pol.fused_imposter is not None
    image = pol.fused_imposter.packed.data_ptr()
    X.assert_same_values(forward_in_canaries(env, pol.fused_imposter, dims[-1]), X.reference_q(first, rows)[0], "the first network")
    for p, t in zip(params, tensors(second)):
        p.data = t  # re-pointed, not written in place
    assert pol.refresh_weights(force=True)
    assert pol.fused_imposter.packed.data_ptr() == image, "re-packed in place"
    X.assert_same_values(forward_in_canaries(env, pol.fused_imposter, dims[-1]), X.reference_q(second, rows)[0], "the second network")
