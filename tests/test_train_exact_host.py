"""CPU checks behind the exact tests of the fused DQN train step (tests/train_exact.py, tests/test_gpu_train_exact.py): the float64
restatement the kernels are judged by equals float64 autograd (pkg.torch_train_step on CPU modules) bit for bit on every one-tile case,
every exact case meets the condition under which any float32 summation order is exact, the cases cover what the GPU test relies on --
conditions on the INPUTS, met by the reference alone -- and the float64 Adam equals torch.optim.Adam.  No kernel is launched here."""
import functools
import importlib

import numpy as np
import pytest
import torch

import qnet_exact as X
import train_exact as T


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@functools.lru_cache(maxsize=None)
def reference_of(case_key):
    """(case, ExactSums, per team np_train_step's results), computed once per case."""
    case = T.one_tile_case(case_key) if case_key in T.ONE_TILE_CASES else T.two_tile_case(case_key)
    ex, want = T.case_reference(case)
    return case, ex, want


ALL_CASES = T.ONE_TILE_CASES + T.TWO_TILE_CASES


def test_the_case_tables():
    assert len(T.ONE_TILE_CASES) == 3 * len(T.STACKS) * 3 and len(set(ALL_CASES)) == len(ALL_CASES)
    assert T.stack_dims("onehot3", "reference") == [[88, 256, 128, 64, 16, 7], [88, 256, 128, 64, 16, 6]]
    assert T.stack_dims("coord1", "ragged") == [[4, 33, 31, 17, 5, 6], [4, 33, 31, 17, 5, 5]]
    for layout in X.LAYOUTS:
        assert T.stack_dims(layout, "caps")[0][1:] == [256, 128, 64, 32, 32]
    assert [T.state_size(k) for k in ("onehot1", "coord1", "onehot3")] == [6, 6, 21]


@pytest.mark.parametrize("case_key", T.ONE_TILE_CASES, ids=T.case_id)
def test_restatement_equals_float64_autograd(pkg, case_key):
    """lr = 0, beta1 = 0: torch's exp_avg after the call is the accumulated gradient.  Every sum is exact, so np_train_step and autograd
    agree bit for bit -- the reference of the GPU test does not rest on the kernels it judges."""
    case, ex, want = reference_of(case_key)
    assert ex.ok
    teams = T.case_teams(case)
    losses, ea, _, prm, steps = T.torch_step(pkg, case["dims"], [tm["params"] for tm in teams], [tm["target"] for tm in teams], case["batch"], case["gamma"],
                                             0.0, (0.0, 0.999), T.EPS)
    for t in range(2):
        grad, loss, n_updates, loss_exact, _ = want[t]
        assert steps[t] == n_updates == sum(len(r) > 0 for _, r in case["lists"][t])
        assert np.array_equal(prm[t], teams[t]["params"])
        for (name, g_), (_, w_) in zip(T.split(case["dims"][t], ea[t]), T.split(case["dims"][t], grad)):
            assert np.array_equal(g_, w_), f"team {t} {name}: max |diff| {np.abs(g_ - w_).max():.3e} of {np.abs(w_).max():.3e}"
        if loss_exact:
            assert losses[t] == loss
        else:
            np.testing.assert_allclose(losses[t], loss, rtol=1e-12)


@pytest.mark.parametrize("case_key", ALL_CASES, ids=T.case_id)
def test_every_summation_order_is_exact(case_key):
    case, ex, want = reference_of(case_key)
    print(f"{T.case_id(case_key)}: worst sum|term|/q = 2^{ex.log2_worst():.1f}; loss sums exact: {[w[3] for w in want if w is not None]}")
    assert ex.ok, f"sum|term|/q reaches 2^{ex.log2_worst():.1f}"
    for t in range(2):
        if want[t] is not None:  # the gradient itself is a float32 value
            assert np.array_equal(want[t][0].astype(np.float32).astype(np.float64), want[t][0])


def test_worst_sums_per_layout():
    worst = {}
    for key in ALL_CASES:
        group = (key[0], "one tile" if key in T.ONE_TILE_CASES else "two tiles")
        worst[group] = max(worst.get(group, 0.0), reference_of(key)[1].log2_worst())
    for (layout, kind), w in sorted(worst.items()):
        print(f"{layout}, {kind} per workgroup: worst sum|term|/q = 2^{w:.1f} of the 2^24 limit")
    assert max(worst.values()) < 24


@pytest.mark.parametrize("case_key", ALL_CASES, ids=T.case_id)
def test_cases_cover_what_the_gpu_test_relies_on(case_key):
    case, _, want = reference_of(case_key)
    b, st = case["batch"], X.directed_states(case["layout"])
    widest = max(d[-1] for d in case["dims"])
    repeats = sum(min(c // 8, max(0, c - widest)) for c in case["counts"])  # (none where a list of 32 rows must take 32 actions)
    assert len(b["idx"]) == case["n"] and len(np.unique(b["idx"])) == case["n"] - repeats and (repeats > 0 or widest == 32), "ring rows repeat"
    assert not np.array_equal(b["idx"], np.sort(b["idx"]))
    assert (case["ring"]["states"][:, 3 * X.LAYOUTS[case["layout"]]["A"]:] == T.JOB_FILL).all()
    for which in ("state_index", "next_index"):  # states no step may follow are real ring contents after an episode ends
        assert (~st["playable"][case[which][b["idx"]]]).any(), which
    for t in range(2):
        for agent, rows in case["lists"][t]:
            assert len(rows) == 0 or T.is_pow2(len(rows))
            if len(rows) and case["enabled"][t]:
                r = b["idx"][rows]
                assert set(b["actions"][r, agent].tolist()) == set(range(case["dims"][t][-1])), (t, agent, "every action index")
                assert 0 < int(b["dones"][r].sum()) < len(r), (t, agent, "done and not-done rows")
                assert set(b["rewards"][r, agent].tolist()) <= set(range(-3, 4))
        if want[t] is None:
            continue
        shares = {name: float((g != 0).mean()) for name, g in T.split(case["dims"][t], want[t][0])}
        print(f"{T.case_id(case_key)} team {t}: non-zero gradient shares {({k: round(v, 2) for k, v in shares.items()})}")
        assert all(v >= 0.10 for k, v in shares.items() if k[0] == "W"), shares
        assert all(v == 1.0 for k, v in shares.items() if k[0] == "a"), shares
    assert [len(r) for _, r in case["lists"][0]] == list(case["counts"]) and [len(r) for _, r in case["lists"][1]] == [case["n"] - c for c in case["counts"]]


def test_ring_rows_are_the_flattened_states():
    for layout in X.LAYOUTS:
        st, A = X.directed_states(layout), X.LAYOUTS[layout]["A"]
        rows = T.ring_rows(layout, st, T.state_size(layout))
        assert rows.dtype == np.float32 and rows.shape == (X.N_STATES, T.state_size(layout))
        for k in (0, 3, 299):
            assert rows[k, :2 * A].tolist() == [float(v) for xy in st["pos"][k] for v in xy] and rows[k, 2 * A:3 * A].tolist() == st["alive"][k].tolist()
        if layout == "coord1":  # the coordinate layout's feature row IS the positions
            assert np.array_equal(rows[:, :2 * A], X.oracle_rows(layout))


def test_float64_adam_equals_torch_adam():
    """adam_f64 against torch.optim.Adam in float64 on the Adam case's gradient, through the four calls' learning rates; and the case's
    eps sits where it matters: within 1/16 .. 16 times sqrt(v) / sqrt(bc2) for at least a quarter of the non-zero-gradient entries."""
    case, ex, want = reference_of(T.ADAM_CASE)
    assert ex.ok and [sum(len(r) > 0 for _, r in case["lists"][t]) for t in range(2)] == [1, 1]
    for t in range(2):
        g = want[t][0]
        eps = T.adam_eps(g)
        share = T.adam_eps_share(g, eps)
        print(f"team {t}: eps = 2^{int(np.log2(eps))}, within 1/16 .. 16 of sqrt(v)/sqrt(bc2) on {100 * share:.0f} % of the non-zero entries; "
              f"{100 * float((g == 0).mean()):.0f} % of the entries have a zero gradient")
        assert share >= 0.25 and (g == 0).any()
        p0 = T.case_teams(case)[t]["params"]
        p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([p], lr=0.0, betas=T.ADAM_BETAS, eps=eps)
        mine = (p0, np.zeros_like(p0), np.zeros_like(p0), 0)
        for lr in T.ADAM_LRS:
            opt.param_groups[0]["lr"] = lr
            p.grad = torch.tensor(g)
            opt.step()
            mine = T.adam_f64(*mine, [g], lr, T.ADAM_BETAS, eps)
            for got_, ref_ in zip(mine[:3], (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])):
                np.testing.assert_allclose(got_, ref_.numpy(), rtol=1e-12, atol=0)
        assert mine[3] == 4 and not np.array_equal(mine[0], p0)
        # the bounds are far below what a wrong formula changes: lr in place of lr / bc1, the smallest slip, moves the update by 1 - bc1 =
        # 2^-4 of itself -- over 100 times the bound wherever eps is within 1/16 .. 16 of the root
        update = mine[0] - p0
        bulk = (g != 0) & (eps >= np.abs(g) / 16) & (eps <= np.abs(g) * 16)
        assert (100 * T.adam_bounds(g, p0, update)[2] <= 2.0 ** -4 * np.abs(update))[bulk].all()
