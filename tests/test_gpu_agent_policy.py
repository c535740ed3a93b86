"""susnet_agent_policy_actions and susnet_state_window_push on the MI355X: with every agent's Q row equal to its env's the per-agent call
is susnet_policy_actions bit for bit (actions, and the whole feed slot of agent_policy_tick_into against policy_tick_into's on a twin env);
per-agent rows at epsilon = 0 against the numpy restatement, ties and signed zeros included; at epsilon = 0.3 every action is the agent's
greedy index or its sample_actions() value and the exploring set is susnet_policy_actions'; the window push bit for bit against its
restatement."""
import importlib

import numpy as np
import pytest
import torch

import spatial_collect_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 70  # two waves, the second one partial
RAW8 = dict(mode="raw", dtype=torch.uint8)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


def make_env(pkg, game, seed=11, batch=B, **kw):
    obs = pkg.ObsConfig(**RAW8)
    if game == "tagging_1v4":
        return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9, obs=obs,
                                                 shuffle_imposter_index=True, **kw)
    return pkg.BatchedFourRoomEnv(2, 6, 4, batch=batch, device=DEV, rng="philox", seed=seed, auto_reset=True, grid_size=9, obs=obs,
                                  shuffle_imposter_index=True, **kw)


def warm_up(env, ticks):
    env.reset()
    for _ in range(ticks):
        env.step(env.sample_actions().clone())


def until_someone_is_dead(env, limit=300):
    """Random ticks until some env has a dead agent (and the tick is not the one after a reset)."""
    env.reset()
    for _ in range(limit):
        env.step(env.sample_actions().clone())
        if bool((~env.alive_agents).any()):
            return
    raise AssertionError("no agent died in the warm-up")


def random_q(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV, dtype=torch.float32)


GAMES = ("tagging_1v4", "base_2v6")


@pytest.fixture(scope="module")
def envs(pkg):
    """One env per game with dead agents in it, and per-env Q rows (shared by the cases below, never stepped by them)."""
    out = {}
    for game in GAMES:
        env = make_env(pkg, game)
        until_someone_is_dead(env)
        gen = torch.Generator(device=DEV).manual_seed(5)
        out[game] = (env, random_q(gen, B, env.n_imposter_actions), random_q(gen, B, env.n_crew_actions))
    return out


# ---- 1. broadcast equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
@pytest.mark.parametrize("crew_net", [True, False])
@pytest.mark.parametrize("mask_dead", [True, False])
@pytest.mark.parametrize("epsilon", [0.0, 0.3])
@pytest.mark.parametrize("game", GAMES)
def test_broadcast_rows_equal_susnet_policy_actions(envs, game, epsilon, mask_dead, crew_net, dtype):
    env, q_imp, q_crew = envs[game]
    A = env.n_agents
    assert bool((~env.alive_agents).any()) and env.n_agents <= 8
    q_crew = q_crew if crew_net else None
    want = env.policy_actions(q_imp, q_crew, out=torch.full((B, A), 99, dtype=dtype, device=DEV), epsilon=epsilon, mask_dead=mask_dead)
    rows_imp = q_imp.unsqueeze(1).expand(B, A, -1).contiguous()
    rows_crew = q_crew.unsqueeze(1).expand(B, A, -1).contiguous() if crew_net else None
    got = env.agent_policy_actions(rows_imp, rows_crew, out=torch.full((B, A), 77, dtype=dtype, device=DEV), epsilon=epsilon, mask_dead=mask_dead)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np_(got), np_(want))
    # the other memory order of the output
    got_ab = env.agent_policy_actions(rows_imp, rows_crew, out=torch.full((A, B), 77, dtype=dtype, device=DEV).t(), epsilon=epsilon, mask_dead=mask_dead)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np_(got_ab), np_(want))


@pytest.mark.parametrize("crew_net", [True, False])
@pytest.mark.parametrize("epsilon", [0.0, 0.3])
@pytest.mark.parametrize("game", GAMES)
def test_feed_slot_of_agent_policy_tick_equals_policy_tick_on_a_twin(pkg, game, epsilon, crew_net):
    """Twin envs, same seed, 6 consecutive ticks across a truncation (auto-resets) with dead agents about."""
    twins = [make_env(pkg, game, seed=23, max_time_steps=20) for _ in range(2)]
    for env in twins:
        warm_up(env, 17)
    a, b = twins
    np.testing.assert_array_equal(np_(a.agent_positions), np_(b.agent_positions))
    A, n_ticks = a.n_agents, 6
    feeds = [env.alloc_feed(n_ticks) for env in twins]
    gen = torch.Generator(device=DEV).manual_seed(9)
    for t in range(n_ticks):
        q_imp = random_q(gen, B, a.n_imposter_actions)
        q_crew = random_q(gen, B, a.n_crew_actions) if crew_net else None
        a.policy_tick_into(feeds[0], t, q_imposter=q_imp, q_crew=q_crew, epsilon=epsilon, mask_dead=True)
        b.agent_policy_tick_into(feeds[1], t, q_imp.unsqueeze(1).expand(B, A, -1).contiguous().view(B * A, -1),
                                 q_crew.unsqueeze(1).expand(B, A, -1).contiguous().view(B * A, -1) if crew_net else None, epsilon=epsilon,
                                 mask_dead=True)
    torch.cuda.synchronize()
    for env in twins:
        env.poll_errors()
    for key in ("actions", "rewards", "done", "truncated", "obs", "term_obs", "roles", "ep_info"):
        x, y = np_(feeds[0][key]), np_(feeds[1][key])
        assert x.tobytes() == y.tobytes(), key
    assert np_(feeds[0]["truncated"]).any(), "the six ticks cross an episode end"
    assert len(np.unique(np_(feeds[0]["actions"]))) > 2


# ---- 2. per-agent rows, epsilon = 0 -----------------------------------------------------------------------------------------------------
def per_agent_rows(gen, n_rows, n):
    """Rows with exact ties (first, middle, last), signed zeros and all-equal rows among random ones."""
    q = random_q(gen, n_rows, n)
    q[0::7] = q[0::7].round()                       # many exact ties among small integers
    q[1::7, :] = 0.5                                # all equal: index 0
    q[2::7, 0], q[2::7, 1] = -0.0, 0.0              # -0.0 then +0.0 at the top ...
    q[2::7, 2:] = -1.0
    q[3::7, 0], q[3::7, 1] = 0.0, -0.0              # ... and the other way round: index 0 both times
    q[3::7, 2:] = -1.0
    q[4::7, n - 1] = q[4::7, n - 2] = 9.0           # the maximum twice at the end: the earlier one
    return q.contiguous()


@pytest.mark.parametrize("mask_dead", [True, False])
@pytest.mark.parametrize("game", GAMES)
def test_per_agent_rows_greedy_equal_the_numpy_restatement(envs, game, mask_dead):
    env = envs[game][0]
    A = env.n_agents
    gen = torch.Generator(device=DEV).manual_seed(17)
    q_imp, q_crew = per_agent_rows(gen, B * A, env.n_imposter_actions), per_agent_rows(gen, B * A, env.n_crew_actions)
    got = env.agent_policy_actions(q_imp, q_crew, out=torch.full((B, A), 77, dtype=torch.int64, device=DEV), epsilon=0.0, mask_dead=mask_dead)
    torch.cuda.synchronize()
    want = U.agent_actions_reference(np_(q_imp).reshape(B, A, -1), np_(q_crew).reshape(B, A, -1), np_(env.imposter_mask), np_(env.alive_agents),
                                     mask_dead=mask_dead)
    np.testing.assert_array_equal(np_(got), want)
    assert len(np.unique(want)) > 3 and (want[np_(env.alive_agents)] != 0).any()
    # rows differ between the agents of an env: the per-env call on agent 0's rows gives something else
    per_env = env.policy_actions(q_imp.view(B, A, -1)[:, 0].contiguous(), q_crew.view(B, A, -1)[:, 0].contiguous(), epsilon=0.0, mask_dead=mask_dead)
    assert not np.array_equal(np_(per_env), want)
    # a random crew at epsilon = 0: the crew's entries are sample_actions()' values
    sampled = np_(env.sample_actions().clone()).astype(np.int64)
    got = env.agent_policy_actions(q_imp, None, out=torch.full((B, A), 77, dtype=torch.int64, device=DEV), epsilon=0.0, mask_dead=mask_dead)
    torch.cuda.synchronize()
    want = U.agent_actions_reference(np_(q_imp).reshape(B, A, -1), None, np_(env.imposter_mask), np_(env.alive_agents), mask_dead=mask_dead,
                                     sampled=sampled)
    np.testing.assert_array_equal(np_(got), want)


# ---- 3. per-agent rows, epsilon = 0.3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_per_agent_rows_exploring_take_the_sampled_value_and_the_same_agents_explore(envs, game):
    env, q_env_imp, q_env_crew = envs[game]
    A, eps = env.n_agents, 0.3
    gen = torch.Generator(device=DEV).manual_seed(29)
    q_imp, q_crew = random_q(gen, B * A, env.n_imposter_actions), random_q(gen, B * A, env.n_crew_actions)
    sampled = np_(env.sample_actions().clone()).astype(np.int64)
    roles, alive = np_(env.imposter_mask), np_(env.alive_agents)
    got = np_(env.agent_policy_actions(q_imp, q_crew, out=torch.full((B, A), 77, dtype=torch.int64, device=DEV), epsilon=eps, mask_dead=False))
    greedy = U.agent_actions_reference(np_(q_imp).reshape(B, A, -1), np_(q_crew).reshape(B, A, -1), roles, alive, mask_dead=False)
    assert ((got == greedy) | (got == sampled)).all()
    # who explored, at the same tick and seed, by the per-env call: rows whose greedy index can never equal the sampled one are not
    # available (any index may be drawn), so compare where the two differ -- and count
    env_greedy = np.where(roles, U.first_argmax(np_(q_env_imp))[:, None], U.first_argmax(np_(q_env_crew))[:, None])
    per_env = np_(env.policy_actions(q_env_imp, q_env_crew, out=torch.full((B, A), 77, dtype=torch.int64, device=DEV), epsilon=eps, mask_dead=False))
    told_a, told_b = greedy != sampled, env_greedy != sampled  # where the outcome tells exploring from acting greedily
    explored_a, explored_b = (got == sampled) & told_a, (per_env == sampled) & told_b
    both = told_a & told_b
    np.testing.assert_array_equal(explored_a[both], explored_b[both])
    frac = explored_a[both].mean()
    assert both.sum() > 0.5 * B * A and 0.15 < frac < 0.45, (both.sum(), frac)
    # epsilon = 1: everybody takes the sampled value
    got = np_(env.agent_policy_actions(q_imp, q_crew, out=torch.full((B, A), 77, dtype=torch.int64, device=DEV), epsilon=1.0, mask_dead=False))
    np.testing.assert_array_equal(got, sampled)


# ---- 4. the window push -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 8])
def test_state_window_push_is_the_restatement_bit_for_bit(pkg, envs, T):
    env = envs["tagging_1v4"][0]
    L = pkg._lib
    S = env.flattened_state_size
    assert S == 41  # odd: dwords + a byte tail per state, rows that start at every alignment
    rng = np.random.default_rng(100 + T)
    window = rng.integers(0, 256, (B, T, S), dtype=np.uint8)
    obs = rng.integers(0, 256, (B, S), dtype=np.uint8)
    done, trunc = rng.random(B) < 0.3, rng.random(B) < 0.3
    assert (done & trunc).any() and (done & ~trunc).any() and (~done & trunc).any() and (~done & ~trunc).any()
    guard = 64
    buf = torch.full((B * T * S + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    w = buf[guard:guard + B * T * S].view(B, T, S)
    w.copy_(torch.from_numpy(window))
    d_obs, d_done, d_trunc = torch.from_numpy(obs).to(DEV), torch.from_numpy(done).to(DEV), torch.from_numpy(trunc).to(DEV)
    with torch.cuda.device(DEV):
        L.check(env.lib.susnet_state_window_push(env._h, w.data_ptr(), T, S, B, d_obs.data_ptr(), d_done.data_ptr(), d_trunc.data_ptr(), env._stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np_(w), U.state_window_push_reference(window, obs, done | trunc))
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[-guard:] == 0xA5).all()), "a byte outside the window was written"
    np.testing.assert_array_equal(np_(d_obs), obs)
