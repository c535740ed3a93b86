"""The fused DQN train step (susnet_dqn_train_step: k_train_select, k_train_grad<ROW>, k_train_adam, k_train_pack) on the MI355X, called by
hand through the C ABI with canaries around every buffer it writes:
  a / b. EXACTLY against the float64 restatement of tests/train_exact.py -- integer networks on the directed states of the three
        compiled-in layouts, dyadic constants, power-of-two counts: every float32 summation order gives the float64 result (asserted on
        the reference), so every gradient word must be EQUAL -- at every stack shape dqn_net accepts, with one tile and with two tiles
        per workgroup;
  c.    Adam through the one k_train_adam, reached from both train steps (this step and susnet_mlp_train_step), against float64 Adam, within bounds
        counted from the kernel's roundings;
  d.    ragged counts and random float weights against torch_train_step on float64 CPU modules, at the project's tolerances.
test_train_exact_host.py states on the CPU that the restatement equals float64 autograd and that the cases cover what is relied on here."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import qnet_exact as X
import train_exact as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def envs(pkg):
    """One handle per layout: the step takes the game's configuration (agents, grid, row size) from it and none of its state."""
    out = {}
    for layout in X.LAYOUTS:
        out[layout] = X.make_env(pkg, layout, 64, device=T.DEV, auto_reset=True, check_errors=False)
        out[layout].reset()
        assert out[layout].flattened_state_size == T.state_size(layout)
    return out


def check_exact(pkg, env, case, packed):
    """lr = 0 and beta1 = 0: exp_avg after the call IS the accumulated gradient.  Everything is an equality."""
    L = pkg._lib
    layout = case["layout"]
    ex, want = T.case_reference(case)
    print(f"worst sum|term|/q = 2^{ex.log2_worst():.1f}; loss sums exact: {[w[3] for w in want if w is not None]}")
    assert ex.ok, f"the construction does not make every summation order exact: sum|term|/q reaches 2^{ex.log2_worst():.1f}"
    teams = T.case_teams(case)
    losses, got = T.fused_abi_step(pkg, env, layout, teams, case, case["gamma"], packed=packed)
    for t in range(2):
        if teams[t] is None:
            continue
        dims = case["dims"][t]
        grad, loss, steps, loss_exact, info = want[t]
        assert got[t]["step"] == steps == sum(len(r) > 0 for _, r in case["lists"][t])
        assert T.same_bits(got[t]["params32"], teams[t]["params"]), "lr = 0: the weights must not move"
        for (name, g_), (_, w_) in zip(T.split(dims, got[t]["exp_avg"]), T.split(dims, grad)):
            bad = np.argwhere(g_ != w_)
            assert len(bad) == 0, (f"team {t} {name}: {len(bad)} of {g_.size} entries differ, first at {bad[0].tolist()}: got {g_[tuple(bad[0])]!r}, "
                                   f"want {w_[tuple(bad[0])]!r}; max |diff| {np.abs(g_ - w_).max():.3e} of {np.abs(w_).max():.3e}")
        if loss_exact:  # every update's mean is a float32 value: the step's float32 accumulation of them, restated
            assert losses[t] == info["loss32"], (t, losses[t], info["loss32"], loss)
        else:
            np.testing.assert_allclose(losses[t], loss, rtol=1e-6)
        if packed:  # the image the policy reads is rewritten from the (unchanged) parameters: bitwise the host packer's
            W, B = case["nets"][t][0]
            image = X.host_pack(L, env._h, layout, (W, B, (case["slope"],) * 4))
            assert T.same_bits(got[t]["image"], image), f"team {t}: the packed image differs from susnet_qnet_pack's in {int((got[t]['image'].view(np.uint32) != image.view(np.uint32)).sum())} words"
    return ex


# ---- a. exact, one tile per workgroup ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_key", T.ONE_TILE_CASES, ids=T.case_id)
def test_exact_one_tile_per_workgroup(pkg, envs, case_key):
    """Both teams, slope 0.5, gamma 0.5, the packed images handed in.  Stacks: the reference's, every width at its cap (67 weight-gradient
    tiles, 512 bias threads), one past / one short of a 32-block, padded widths, all ones.  n = 64 split between two agents (on onehot3 the
    third agent's imposter update is empty and its crew list is the whole batch), n = 64 with agent 0 always the imposter (the production
    1v1 case), n = 128 on G = 4 workgroups of which two get no tile of a 64-row list and write zero partials."""
    check_exact(pkg, envs[case_key[0]], T.one_tile_case(case_key), packed=True)


# ---- b. exact, two tiles per workgroup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_key", T.TWO_TILE_CASES, ids=T.case_id)
def test_exact_two_tiles_per_workgroup(pkg, envs, case_key):
    """n = 16384: G = 256 workgroups, and a list of 16384 rows (agent 0's imposter rows on onehot1, agent 2's crew rows on onehot3) gives
    every workgroup two tiles, summed in the register accumulators.  Slope 1, gamma 1, two weights per unit: what keeps every sum exact
    at this size (slope 0.5 does not, on any layout); the reference stack runs the crew team alone.  The coordinate layout is exact at
    this size under no setting tried (coordinates up to 8 multiply through: 2^24.7 at best): test_ragged_counts_against_float64 covers
    it at n = 16384 against float64."""
    check_exact(pkg, envs[case_key[0]], T.two_tile_case(case_key), packed=False)


# ---- c. Adam, from both train steps ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adam_reference():
    """The Adam case, its exact gradient per team (one update per call) and, per team, eps and float64 Adam after each of the four calls."""
    case = T.one_tile_case(T.ADAM_CASE)
    ex, want = T.case_reference(case)
    assert ex.ok
    teams = T.case_teams(case)
    ref = []
    for t in range(2):
        grad, updates = want[t][0], want[t][4]["updates"]
        assert len(updates) == 1 and np.array_equal(np.cumsum(updates, axis=0)[-1], grad)
        eps = T.adam_eps(grad)
        assert T.adam_eps_share(grad, eps) >= 0.25, "eps must be of the root's size where it is to matter"
        states, state = [], (teams[t]["params"], np.zeros_like(grad), np.zeros_like(grad), 0)
        for lr in T.ADAM_LRS:
            state = T.adam_f64(*state, list(np.cumsum(updates, axis=0)), lr, T.ADAM_BETAS, eps)
            states.append(state)
        ref.append(dict(grad=grad, eps=eps, states=states))
    return case, teams, ref


@pytest.mark.parametrize("step_fn", ["susnet_dqn_train_step", "susnet_mlp_train_step"])
def test_adam_against_float64(pkg, envs, step_fn):
    """Four calls on one exact batch (n = 64, agent 0 always the imposter: one update per team and call), betas (0.5, 0.75), eps a power
    of two at the median gradient magnitude, the Adam state carried from call to call.  Calls 1 - 3 with lr = 0: step = k, the
    parameters bitwise unchanged, exp_avg and exp_avg_sq against the float64 recurrences on the exact gradient.  Call 4 with lr = 2^-6:
    the parameters against p - lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) in float64.
    The bounds are counted, not measured (train_exact.adam_bounds; u = 2^-24): |m - m64| <= 4 u |g| (2 roundings a step, the carried
    error halving), |v - v64| <= 9 u g^2 (3 roundings a step, the carried error shrinking by 0.75), |p - p64| <= 25 u |update| + u |p|
    (relative: m 4.3 u, the root of v 6.6 u, sqrtf 2 u, sqrt(bc2) u, the division 2 u, + eps u, lr / bc1 u, m / denom 2 u, the product u
    = 20.9 u, taken as 24 u; the final add u (|p| + |update|)).  Where the gradient is zero m = v = 0 and p is unchanged, bit for bit.
    lr in place of lr / bc1 is off by 2^-4 |update| = 4e4 times that bound, eps inside the root or a (1 - beta2) slip by more."""
    case, teams0, ref = adam_reference()
    env = envs["onehot1"]
    teams = [dict(tm, betas=T.ADAM_BETAS, eps=ref[t]["eps"]) for t, tm in enumerate(teams0)]
    for k, lr in enumerate(T.ADAM_LRS, start=1):
        for tm in teams:
            tm["lr"] = lr
        if step_fn == "susnet_dqn_train_step":
            _, got = T.fused_abi_step(pkg, env, "onehot1", teams, case, case["gamma"], packed=False)
        else:
            _, got = T.abi_step(pkg, env, teams, case["batch"], case["gamma"])
        for t in range(2):
            g = ref[t]["grad"]
            p64, m64, v64, step = ref[t]["states"][k - 1]
            p0 = teams0[t]["params"]
            bm, bv, bp = T.adam_bounds(g, p0, p64 - p0)
            assert got[t]["step"] == step == k
            em, ev, ep = np.abs(got[t]["exp_avg"] - m64), np.abs(got[t]["exp_avg_sq"] - v64), np.abs(got[t]["params"] - p64)
            live = g != 0
            print(f"call {k} team {t}: worst error / bound: exp_avg {np.max(em[live] / bm[live]):.3f}, exp_avg_sq {np.max(ev[live] / bv[live]):.3f}"
                  + (f", params {np.max(ep[live] / bp[live]):.3f}" if lr else ""))
            assert (em <= bm).all(), f"call {k} team {t} exp_avg: {int((em > bm).sum())} entries beyond 4 u |g|, worst {np.max(em[live] / bm[live]):.3g} bounds"
            assert (ev <= bv).all(), f"call {k} team {t} exp_avg_sq: {int((ev > bv).sum())} entries beyond 9 u g^2, worst {np.max(ev[live] / bv[live]):.3g} bounds"
            assert not got[t]["exp_avg"][~live].any() and not got[t]["exp_avg_sq"][~live].any()
            if lr == 0.0:
                assert T.same_bits(got[t]["params32"], p0), f"call {k}: lr = 0 must leave the parameters bit for bit"
            else:
                assert T.same_bits(got[t]["params32"][~live], p0[~live]), "a zero gradient must leave its parameter bit for bit"
                assert (ep <= bp).all(), f"call {k} team {t} params: {int((ep > bp).sum())} entries beyond the bound, worst {np.max(ep[live] / bp[live]):.3g} bounds"
                assert (np.abs(p64 - p0)[live] > 0).all() and (got[t]["params"] != p0)[live].mean() > 0.9, "the step moved the parameters"
            teams[t].update(params=got[t]["params"], exp_avg=got[t]["exp_avg"], exp_avg_sq=got[t]["exp_avg_sq"], step=got[t]["step"])


# ---- d. ragged counts, against float64 ---------------------------------------------------------------------------------------------------
RAGGED_CASES = [(layout, stack, n) for layout in ("onehot1", "onehot3", "coord1") for stack in ("ragged", "reference") for n in (1, 31, 33, 65)]
RAGGED_CASES += [("coord1", "ragged", 16384), ("coord1", "reference", 16384)]


@pytest.mark.parametrize("layout,stack,n", RAGGED_CASES, ids=[f"{l}-{s}-{n}" for l, s, n in RAGGED_CASES])
def test_ragged_counts_against_float64(pkg, envs, layout, stack, n):
    """What exactness cannot cover: counts that are no powers of two (random imposters, ragged last tiles, n = 1) and the coordinate layout
    at n = 16384.  Random float weights (pkg.MLP, seeded) on the directed states; the reference is torch_train_step on float64 CPU modules
    fed the oracle's feature rows.  Tolerances are the project's: losses rtol 1e-4, the first call's gradient (exp_avg) within 1e-4 of each
    tensor's max-abs, step counts exact.  The float32 torch path's own error against the same float64 result is printed beside the
    kernel's.  Measured on an MI355X over the 26 cases: the kernel's worst tensor within 4.4e-5 of max-abs (float32 torch: 5.6e-5), losses
    within 3.4e-7 relative (float32 torch: 1.5e-7) -- no case needed more than the tolerances above."""
    case = T.float_case(layout, n, seed=1000 + n)
    dims_pair = T.stack_dims(layout, stack)
    init = []
    for t, dims in enumerate(dims_pair):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(n + t)
            init.append(torch.cat([p.detach().reshape(-1) for p in pkg.MLP(dims).parameters()]).double().numpy())
    l64, ea64, _, _, st64 = T.torch_step(pkg, dims_pair, init, init, case["batch"], 0.9, 1e-3, T.BETAS, T.EPS, torch.float64)
    l32, ea32, _, _, _ = T.torch_step(pkg, dims_pair, init, init, case["batch"], 0.9, 1e-3, T.BETAS, T.EPS, torch.float32)
    teams = [dict(dims=d, params=init[t], target=init[t], lr=1e-3, betas=T.BETAS, eps=T.EPS) for t, d in enumerate(dims_pair)]
    losses, got = T.fused_abi_step(pkg, envs[layout], layout, teams, case, 0.9, packed=False)
    worst = [0.0, 0.0]
    for t, d in enumerate(dims_pair):
        assert got[t]["step"] == st64[t] == sum(len(r) > 0 for _, r in case["lists"][t])
        for (name, g_), (_, r_), (_, f_) in zip(T.split(d, got[t]["exp_avg"]), T.split(d, ea64[t]), T.split(d, ea32[t])):
            scale = max(float(np.abs(r_).max()), 1e-30)
            err, err32 = float(np.abs(g_ - r_).max()) / scale, float(np.abs(f_ - r_).max()) / scale
            worst = [max(worst[0], err), max(worst[1], err32)]
            print(f"team {t} {name}: kernel {err:.2e}, float32 torch {err32:.2e} of max-abs")
            assert err <= 1e-4 or float(np.abs(r_).max()) == 0.0 == float(np.abs(g_).max()), f"team {t} {name}: first-step gradient off by {err:.2e}"
    rel = lambda a: np.abs(a - l64) / np.maximum(np.abs(l64), 1e-30)
    print(f"worst tensor: kernel {worst[0]:.2e}, float32 torch {worst[1]:.2e} of max-abs; losses: kernel rel {rel(losses)}, float32 torch rel {rel(l32)}")
    np.testing.assert_allclose(losses, l64, rtol=1e-4)
    assert math.isfinite(float(losses.sum()))
