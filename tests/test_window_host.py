"""CPU-only checks of the state-window fixtures (tests/golden/window/wcollect_*.npz: the reference trainer's collection loop at
sequence_length T > 1, tests/golden/generate_collect_window.py) and of the push rule's restatement the package keeps
(``policy.window_push_reference``: what ``susnet_window_push`` is compared with on the GPU).

The feature rows come from the CPU oracle's FlatFeaturizer (``OracleBatch.obs_flat``, pinned to the reference's featurizers by the
feat_* fixtures): the package's ``FlatFeaturizer`` runs its HIP kernel and needs the GPU.  They are checked against the rows the reference's own
featurizer produced in the run (``window_feats``) first, so the restatement below is held to the reference's features either way."""
import glob
import importlib
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN_DIR, load_golden

WINDOW_DIR = os.path.join(GOLDEN_DIR, "window")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WINDOW_DIR, "wcollect_*.npz")))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_the_three_cases_are_there():
    metas = {n: load_golden(os.path.join(WINDOW_DIR, n + ".npz"))["meta"] for n in NAMES}
    kinds = sorted((m["class"], m["trajectory_size"]) for m in metas.values())
    assert kinds == [("base", 2), ("base", 3), ("itg", 2)], kinds
    for name, m in metas.items():
        assert os.path.getsize(os.path.join(WINDOW_DIR, name + ".npz")) < (1 << 20)
        assert m["imposter_dims"][0] == m["crew_dims"][0] == m["trajectory_size"] * m["n_features"], "the networks read the flattened window"
    wrapped = [m for m in metas.values() if m["num_steps"] > m["max_size"]]
    assert wrapped and all(m["size"] == m["max_size"] and m["idx"] == m["num_steps"] % m["max_size"] for m in wrapped), "one ring wraps"
    assert any(m["class"] == "itg" and m["episodes_ended"] >= 15 for m in metas.values()), "episodes that end by kills: done rows"


def chronological(g):
    """The ring's rows in the order they were added (a wrapped ring starts at its cursor)."""
    m = g["meta"]
    n = m["size"]
    return (m["idx"] + np.arange(n)) % n if m["num_steps"] > m["max_size"] else np.arange(n)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_rows_obey_the_window_rules(name):
    """train.py:388-389 within a row (the next window is the window rolled by one), 441-445 / 318-322 between rows (after a transition that
    ended its episode the window holds one state T times; otherwise it is the stored next window)."""
    g = load_golden(os.path.join(WINDOW_DIR, name + ".npz"))
    order = chronological(g)
    states, nxt, ended = g["states"][order], g["next_states"][order], g["ended"][order].astype(bool)
    T = g["meta"]["trajectory_size"]
    assert states.shape[1] == T and T > 1
    np.testing.assert_array_equal(nxt[:, :-1], states[:, 1:])
    assert ended.sum() == g["meta"]["windows_refilled"] > 5 and not ended.all()
    assert (g["dones"][order].reshape(-1).astype(bool) <= ended).all(), "a done row ended its episode"
    for r in range(len(order) - 1):
        if ended[r]:
            assert (states[r + 1] == states[r + 1][0]).all(), f"row {r + 1}: a fresh episode's window is its first state {T} times"
        else:
            np.testing.assert_array_equal(states[r + 1], nxt[r], err_msg=f"row {r + 1}")
    assert any((states[r + 1][-1] != nxt[r][-1]).any() for r in np.flatnonzero(ended[:-1])), "the terminal state is not the fresh one"


@pytest.mark.parametrize("name", NAMES)
def test_fixture_margin_condition(name):
    """No action of the run can be flipped by a float32 summation-order difference: the smallest argmax margin is more than 100 times the
    kernels' tolerance against torch, 2e-5 x the largest |Q|."""
    m = load_golden(os.path.join(WINDOW_DIR, name + ".npz"))["meta"]
    assert m["largest_abs_q"] > 0
    assert m["smallest_argmax_margin"] > 100 * (2e-5 * m["largest_abs_q"])


def oracle_features(oracle_mod, g, raw):
    """FlatFeaturizer rows ``[n, F]`` of flattened states ``raw [n, S]`` (base.py:234: x0, y0, .., alive.., job x, y.., job done..)."""
    meta = g["meta"]
    n, A = len(raw), meta["n_agents"]
    ob = oracle_mod.OracleBatch(oracle_mod.config_from_fixture_meta(meta), n)
    ob.set_philox(1, 0, 0)
    ob.reset()
    J = ob.J
    imp = np.zeros(A, dtype=np.uint8)
    imp[int(g["imposters"][0, 0])] = 1
    assert (g["imposters"] == g["imposters"][0, 0]).all(), "one imposter, fixed index"
    for k in range(n):
        row = raw[k].astype(np.int64)
        ob.set_state(k, pos=row[:2 * A].reshape(A, 2), alive=row[2 * A:3 * A], jobpos=row[3 * A:3 * A + 2 * J].reshape(J, 2),
                     jobdone=row[3 * A + 2 * J:3 * A + 3 * J], imp_mask=imp)
    feats = ob.obs_flat(meta["components"])
    assert feats.shape == (n, meta["n_features"]) and feats.dtype == np.float32
    return feats


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("backend", ["numpy", "torch"])
def test_push_restatement_reproduces_the_reference_feature_windows(pkg, oracle_mod, name, backend):
    """The restated push rule, driven by the run's episode flags and fed ONE fresh feature row per tick, reproduces the features of every
    window the reference's networks acted on -- all T states of it, which the reference featurizes anew every tick."""
    g = load_golden(os.path.join(WINDOW_DIR, name + ".npz"))
    order = chronological(g)
    states, ended = g["states"][order], g["ended"][order]
    n, T, S = states.shape
    F = g["meta"]["n_features"]
    feats = oracle_features(oracle_mod, g, states.reshape(n * T, S)).reshape(n, T * F)  # features(states[r]) flattened, oldest state first
    np.testing.assert_array_equal(feats, g["window_feats"][order].astype(np.float32), err_msg="the oracle's rows vs the reference featurizer's")
    conv = (lambda x: torch.from_numpy(np.ascontiguousarray(x))) if backend == "torch" else np.ascontiguousarray
    back = (lambda x: x.numpy()) if backend == "torch" else (lambda x: x)
    window = conv(feats[0])[None]
    for r in range(n - 1):
        fresh = conv(feats[r + 1][(T - 1) * F:])[None]  # the newest state of the next window: the state after the tick / the fresh first state
        flag = conv(ended[r:r + 1])
        window = pkg.policy.window_push_reference(window, fresh, done=flag) if r % 2 else pkg.policy.window_push_reference(window, fresh, None, flag)
        assert back(window).view(np.int32).tolist() == feats[r + 1:r + 2].view(np.int32).tolist(), f"window after row {r} (ended: {int(ended[r])})"


def test_push_restatement_moves_bit_patterns(pkg):
    rng = np.random.default_rng(5)
    n, T, F = 7, 3, 5
    src = rng.integers(-2**31, 2**31 - 1, size=(n, T * F), dtype=np.int64).astype(np.int32).view(np.float32)
    fresh = rng.integers(-2**31, 2**31 - 1, size=(n, F), dtype=np.int64).astype(np.int32).view(np.float32)
    fresh[0, 0], fresh[1, 1] = -0.0, np.float32(np.nan)
    done = np.array([1, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    trunc = np.array([0, 0, 1, 1, 0, 0, 0], dtype=bool)
    want = np.where((done.astype(bool) | trunc)[:, None], np.tile(fresh.view(np.int32), (1, T)),
                    np.concatenate([src.view(np.int32)[:, F:], fresh.view(np.int32)], 1))
    got_np = pkg.policy.window_push_reference(src, fresh, done, trunc)
    got_t = pkg.policy.window_push_reference(torch.from_numpy(src), torch.from_numpy(fresh), torch.from_numpy(done), torch.from_numpy(trunc))
    assert got_np.dtype == np.float32 and got_t.dtype == torch.float32
    assert got_np.view(np.int32).tolist() == want.tolist() == got_t.numpy().view(np.int32).tolist()
    none = pkg.policy.window_push_reference(src, fresh)
    assert none.view(np.int32).tolist() == np.concatenate([src.view(np.int32)[:, F:], fresh.view(np.int32)], 1).tolist()
