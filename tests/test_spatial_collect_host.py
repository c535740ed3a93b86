"""CPU-only checks of the SpatialDQN collection path: the reference trainer's own runs (tests/golden/spatial_collect/) load, stay under the
size cap and keep their margin condition; the numpy restatements the GPU tests share reproduce them (the per-agent acting rule on the
stored Q rows, the window push on the stored states); and what the Python layer decides without a device."""
import importlib
import inspect
import os

import numpy as np
import pytest

import spatial_collect_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_both_cases_of_the_issue_are_there():
    assert U.CASES == ["base14_1v2_j4_persp_t3", "base_1v3_j5_global_t2_wrap"]


@pytest.mark.parametrize("name", U.CASES)
def test_fixture_loads_and_keeps_its_condition(name):
    path = os.path.join(U.SPATIAL_COLLECT_DIR, name + ".npz")
    assert os.path.getsize(path) < U.SIZE_CAP
    g = U.load_case(name)
    meta = g["meta"]
    assert meta["smallest_argmax_margin"] > U.MARGIN_FACTOR * U.KERNEL_TOLERANCE * meta["largest_abs_q"]
    T, S, A, ticks, n = meta["trajectory_size"], meta["state_size"], meta["n_agents"], meta["num_steps"], meta["size"]
    assert g["states"].shape == g["next_states"].shape == (n, T, S) and g["actions"].shape == g["rewards"].shape == (n, A)
    assert g["taken"].shape == g["alive"].shape == g["imposter_mask"].shape == (ticks, A) and g["ended"].shape == (ticks,)
    assert g["q_imposter"].shape == (ticks, A, meta["n_actions"]["imposter"]) and g["q_crew"].shape == (ticks, A, meta["n_actions"]["crew"])
    assert g["q_imposter"].dtype == g["q_crew"].dtype == np.float32
    assert g["fresh"].shape == (ticks, S) and g["first_state"].shape == (S,)
    assert n == min(ticks, meta["max_size"]) and meta["idx"] == ticks % meta["max_size"]
    assert meta["windows_refilled"] > 0
    # the margin the meta states is the one of the stored rows: living agents, their own team's row
    own = np.where(g["imposter_mask"].astype(bool)[..., None], np.pad(g["q_imposter"], ((0, 0), (0, 0), (0, max(0, g["q_crew"].shape[2] - g["q_imposter"].shape[2]))), constant_values=-np.inf),
                   np.pad(g["q_crew"], ((0, 0), (0, 0), (0, max(0, g["q_imposter"].shape[2] - g["q_crew"].shape[2]))), constant_values=-np.inf))
    top = np.sort(own, axis=-1)
    margins = (top[..., -1] - top[..., -2])[g["alive"].astype(bool)]
    assert float(margins.min()) == pytest.approx(meta["smallest_argmax_margin"], abs=0.0)


def test_the_wrapped_case_wraps_and_has_dead_agents():
    g = U.load_case("base_1v3_j5_global_t2_wrap")
    meta = g["meta"]
    assert meta["num_steps"] > meta["max_size"] and meta["featurizer"] == "GlobalFeaturizer" and meta["trajectory_size"] == 2
    assert meta["dead_agent_ticks"] > 0 and int((g["alive"] == 0).sum()) == meta["dead_agent_ticks"]
    p = U.load_case("base14_1v2_j4_persp_t3")["meta"]
    assert p["featurizer"] == "PerspectiveFeaturizer" and p["trajectory_size"] == 3 and len(p["grid_used"]) == 14


@pytest.mark.parametrize("name", U.CASES)
def test_the_acting_rule_restated_reproduces_the_actions_taken(name):
    g = U.load_case(name)
    want = g["taken"].astype(np.int64)
    got = U.agent_actions_reference(g["q_imposter"], g["q_crew"], g["imposter_mask"], g["alive"], mask_dead=True)
    np.testing.assert_array_equal(got, want)
    # and the ring's action rows are the last `size` ticks of it, at tick % max_size
    meta = g["meta"]
    for t in range(meta["num_steps"] - meta["size"], meta["num_steps"]):
        np.testing.assert_array_equal(g["actions"][t % meta["max_size"]], want[t])


def test_first_argmax_rule_on_ties_and_signed_zeros():
    q = np.array([[1.0, 3.0, 3.0, 2.0], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0], [-1.0, -1.0, -1.0, -1.0], [2.0, 1.0, 2.0, 5.0]], dtype=np.float32)
    np.testing.assert_array_equal(U.first_argmax(q), [1, 0, 0, 0, 3])
    np.testing.assert_array_equal(U.first_argmax(q), np.argmax(q, axis=-1))


@pytest.mark.parametrize("name", U.CASES)
def test_the_window_push_restated_reproduces_the_ring_windows(name):
    """From the run's first state T times, pushed tick by tick with the stored post-tick states and `ended` flags: the window before tick t is
    the ring row's `states`, and its `next_states` is that window shifted by one (the last slot is the state the step returned, which is
    `fresh` where the episode went on)."""
    g = U.load_case(name)
    meta = g["meta"]
    T, ticks, M = meta["trajectory_size"], meta["num_steps"], meta["max_size"]
    window = np.repeat(g["first_state"][None, None, :], T, axis=1)  # [1, T, S]
    checked = 0
    for t in range(ticks):
        if t >= ticks - meta["size"]:
            row = t % M
            np.testing.assert_array_equal(window[0], g["states"][row], err_msg=f"states of tick {t}")
            np.testing.assert_array_equal(window[0, 1:], g["next_states"][row][:-1], err_msg=f"next_states of tick {t}")
            if not g["ended"][t]:
                np.testing.assert_array_equal(g["fresh"][t], g["next_states"][row][-1])
            checked += 1
        window = U.state_window_push_reference(window, g["fresh"][t][None], g["ended"][t:t + 1])
    assert checked == meta["size"]


def test_window_push_reference_rules():
    w = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    obs = -np.ones((2, 4), dtype=w.dtype)
    out = U.state_window_push_reference(w, obs, [0, 1])
    np.testing.assert_array_equal(out[0], np.concatenate([w[0, 1:], obs[:1]]))
    np.testing.assert_array_equal(out[1], np.repeat(obs[1:2], 3, axis=0))
    one = U.state_window_push_reference(w[:, :1], obs, [0, 0])  # T = 1: the window is the new state
    np.testing.assert_array_equal(one[:, 0], obs)


def test_python_layer_names_the_spatial_form(pkg):
    sig = inspect.signature(pkg.BatchedFourRoomEnv.agent_policy_tick_into)
    assert list(sig.parameters)[1:] == ["feed", "t", "q_imposter", "q_crew", "epsilon", "mask_dead"]
    assert sig.parameters["q_crew"].default is None and sig.parameters["epsilon"].default == 0.0 and sig.parameters["mask_dead"].default is True
    W = pkg.policy.WindowedPolicyRollout
    for name in ("reset_window", "load_window", "push", "q_rows", "refresh_weights", "sequence_length"):
        assert hasattr(W, name), name
    assert "featurizer" in inspect.signature(pkg.train_loop.run_experiment).parameters
    assert "featurizer" in inspect.signature(pkg.train_loop.evaluate).parameters
    assert "MLP-only" in pkg.train_loop.run_sweep.__doc__
    assert "spatial_dqn" in pkg.train_loop.evaluate_checkpoints.__doc__


def test_served_by_kernels_knows_the_per_agent_kind(pkg):
    P = pkg.policy

    class Flat:  # what served_by_kernels reads of a PolicyRollout
        fused_imposter, fused_crew, dense_imposter, dense_crew, crew_model = object(), None, None, None, None

    assert P.served_by_kernels(Flat()) == (True, True, False) and not P.acts_per_agent(Flat())
    w = object.__new__(P.WindowedPolicyRollout)  # (no env: only the attributes the decision reads)
    w.spatial_imposter, w.spatial_crew, w.crew_model = object(), None, None
    assert P.acts_per_agent(w) and P.served_by_kernels(w) == (True, True, False)  # a crew without a model is random: served
    w.crew_model = object()
    assert P.served_by_kernels(w) == (True, False, False)  # a crew model the spatial kernels do not serve
    w.spatial_crew, w.spatial_imposter = object(), None
    assert P.served_by_kernels(w) == (False, True, False)
    assert w.refresh_weights() is False and w.refresh_weights(force=True) is False


def test_block_actor_decides_the_form_once(pkg):
    P = pkg.policy

    class Env:  # what the decision reads of an env
        def __init__(self, batch, one_kernel=True):
            self.batch, self.flattened_state_size, self.one_kernel, self.asked = batch, 21, one_kernel, []

        def supports_qnet_policy_step(self, net, net_crew, epsilon):
            self.asked.append((net, net_crew, epsilon))
            return self.one_kernel

    class Fused:
        fused_imposter, fused_crew, dense_imposter, dense_crew, crew_model = "imp", None, None, None, None

    class Dense(Fused):
        fused_imposter, dense_imposter, sequence_length = None, object(), 2

    spatial = object.__new__(P.WindowedPolicyRollout)
    spatial.spatial_imposter, spatial.spatial_crew, spatial.crew_model, spatial.T = object(), None, None, 2

    def form(env, policy, n_block, **kw):
        actor = P.BlockActor(env, policy, 0.25, True, n_block, **kw)
        assert actor.last is None and actor.n_block == n_block and (actor.imp_served, actor.crew_served) == (True, True)
        assert actor.refresh_obs_after == (actor.form in ("dense", "per_agent"))
        return actor.form

    aligned, unaligned = Env(16), Env(3)
    assert (16 * 21) % 16 == 0 and (3 * 21) % 16 != 0
    assert form(aligned, Fused(), 4) == "block"
    assert aligned.asked == [("imp", None, 0.25)]
    assert form(unaligned, Fused(), 4) == "ticks"
    assert form(unaligned, Fused(), 1) == "block"  # one slot: nothing to align
    unserved = Env(16, one_kernel=False)
    assert form(unserved, Fused(), 4) == "ticks"
    assert P.BlockActor(unserved, Fused(), 0.0, True, 4).one_kernel is False and P.BlockActor(aligned, Fused(), 0.0, True, 4).one_kernel is True
    n_asked = len(aligned.asked)
    assert form(aligned, Fused(), 4, one_launch_per_block=False) == "ticks"
    assert len(aligned.asked) == n_asked  # the env is asked where the answer is used

    class Unserved(Fused):
        fused_imposter = None

    lost = P.BlockActor(aligned, Unserved(), 0.0, True, 4)
    assert (lost.imp_served, lost.form, lost.one_kernel) == (False, "ticks", False) and len(aligned.asked) == n_asked
    assert form(aligned, Dense(), 4) == "dense" and form(aligned, spatial, 4) == "per_agent"
    assert len(aligned.asked) == n_asked  # only a fused policy asks the env
    assert P.BlockActor(aligned, Dense(), 0.0, True, 4).windowed and not P.BlockActor(aligned, spatial, 0.0, True, 4).windowed
    assert P.acting_kind(Fused()) == ("fused", True, True) and P.acting_kind(Dense()) == ("dense", True, True)
    assert P.acting_kind(spatial) == ("per_agent", True, True)
    # the shared refusals: the words behind `who:` are one text
    tape = type("E", (), dict(rng_kind="numpy", n_imposter_actions=17, n_crew_actions=5))()
    with pytest.raises(ValueError, match="^x: a random crew draws from the production stream: build the env with rng='philox'$"):
        P.check_random_crew_stream("x", tape, Fused())
    with pytest.raises(ValueError, match="^x: susnet_policy_step takes at most 16 actions per team, this game has 17 / 5: tail$"):
        P.check_policy_step_actions("x", tape, ": tail")
    tape.rng_kind, tape.n_imposter_actions = "philox", 16
    P.check_random_crew_stream("x", tape, Fused())
    P.check_policy_step_actions("x", tape)


def test_docs_no_longer_say_the_path_stays_out():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "susnet_agent_policy_actions" in text, doc
        assert "for a `SpatialDQN` stay out" not in text and "do not use it yet" not in text, doc
