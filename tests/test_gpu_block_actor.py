"""evaluate() against DeviceReplayBuffer.collect on the MI355X, for the acting forms of a PolicyRollout: the fused block in one launch,
fused ticks (a batch whose observation slots are not 16-byte aligned), dense ticks at T = 1 and on a window of T = 2 states.  Two envs of
one seed: one goes through evaluate(), its twin is reset and driven by collect() block by block, every block's feed into an EpisodeLog;
the two summaries must be the same numbers.  (The per-agent form has test_gpu_spatial_collect.py::test_evaluate_equals_a_hand_fed_episode_log.)"""
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
EPSILON, GAMMA = 0.2, 0.9


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def fused_1v2(pkg, batch, max_time_steps):
    """The compiled-in 1v2 14x14 4-job game on a compiled-in feature layout: a reference MLP against a random crew is one kernel per tick."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device=DEV, rng="philox", seed=11, auto_reset=True, grid_size=14,
                                  shuffle_imposter_index=True, max_time_steps=max_time_steps, obs=pkg.ObsConfig("flat", COMPS3))


def tagging_1v4(pkg, batch, max_time_steps):
    """A game without a fused path: the dense kernel serves it."""
    return pkg.BatchedFourRoomEnvWithTagging(1, 4, 5, batch=batch, device=DEV, rng="philox", seed=11, auto_reset=True, grid_size=9,
                                             max_time_steps=max_time_steps, obs=pkg.ObsConfig("flat", ["onehot_pos"]))


def seeded_mlp(pkg, dims, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = pkg.MLP(dims)
    return model.to(DEV).eval()


def assert_evaluate_equals_collect(pkg, make_env, models, comps, n_ticks, block_ticks, T=1):
    imp, crew = models
    env, twin = make_env(), make_env()
    got = pkg.evaluate(env, imp, crew, comps, n_ticks, epsilon=EPSILON, block_ticks=block_ticks, mask_dead=True, gamma=GAMMA, sequence_length=T)
    # the twin: collect() block by block, ticks_per_append = block_ticks, every block's last_feed into a log
    policy = pkg.PolicyRollout(twin, imp, crew, components=list(comps), epsilon=EPSILON, mask_dead=True, dense=True, sequence_length=T)
    ring = pkg.DeviceReplayBuffer(twin.batch * n_ticks, twin.flattened_state_size, T, twin.n_agents, twin.n_imposters, device=twin.device)
    twin.reset()
    log = pkg.EpisodeLog(twin, gamma=GAMMA, capacity=twin.batch * n_ticks)
    for t0 in range(0, n_ticks, block_ticks):
        n = min(block_ticks, n_ticks - t0)
        assert ring.collect(twin, policy, n, epsilon=EPSILON, mask_dead=True, ticks_per_append=block_ticks) == n * twin.batch
        feed, filled = ring.last_feed
        assert filled == n
        log.update(feed, filled, tick_base=t0)
    want = pkg.train_loop.summarize_episodes(log.records(), ticks=n_ticks)
    assert got["episodes"] >= 2 and want["episodes"] >= 2 and got["dropped"] == 0
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key] or (math.isnan(got[key]) and math.isnan(want[key])), key
    # (short episodes end by truncation with equal returns whatever was done: the states the two runs end in tell their actions apart)
    assert torch.equal(env.observe(pkg.ObsConfig("raw", dtype=torch.uint8)), twin.observe(pkg.ObsConfig("raw", dtype=torch.uint8)))
    assert torch.equal(env.rng_cursor(), twin.rng_cursor()) and torch.equal(env.lifetime_totals(), twin.lifetime_totals())
    return env, policy


@pytest.mark.parametrize("B,aligned", [(16, True), (3, False)])
def test_fused_evaluate_equals_collect(pkg, B, aligned):
    """10 ticks in blocks of 4 (the last block is short), max_time_steps = 3: every env ends at least three episodes.  B = 16: the block in
    ONE launch; B = 3: B * state_size is no multiple of 16, so both sides act tick by tick."""
    make_env = lambda: fused_1v2(pkg, B, max_time_steps=3)
    probe = make_env()
    imp = pkg.policy.reference_imposter_mlp(probe, COMPS3, seed=3)
    net = pkg.policy.pack_mlp(probe, imp, COMPS3)
    assert net is not None and probe.supports_qnet_policy_step(net, None, EPSILON), "the game must be served by the one-kernel tick"
    assert ((B * probe.flattened_state_size) % 16 == 0) == aligned, (B, probe.flattened_state_size)
    env, policy = assert_evaluate_equals_collect(pkg, make_env, (imp, None), COMPS3, n_ticks=10, block_ticks=4)
    assert policy.fused_imposter is not None and policy.dense_imposter is None


@pytest.mark.parametrize("T", [1, 2])
def test_dense_evaluate_equals_collect(pkg, T):
    """7 ticks in blocks of 3, max_time_steps = 2: episodes end inside blocks and at their last slot, so at T = 2 the window push reads an
    ended flag across a block boundary; every env ends three episodes.  T = 1 against a random crew, T = 2 with a crew network."""
    B = 5
    make_env = lambda: tagging_1v4(pkg, B, max_time_steps=2)
    probe = make_env()
    F = probe.obs.shape[-1]
    imp = seeded_mlp(pkg, [T * F, 8, probe.n_imposter_actions], seed=3)
    crew = seeded_mlp(pkg, [T * F, 8, probe.n_crew_actions], seed=4) if T > 1 else None
    env, policy = assert_evaluate_equals_collect(pkg, make_env, (imp, crew), ["onehot_pos"], n_ticks=7, block_ticks=3, T=T)
    assert policy.fused_imposter is None and policy.dense_imposter is not None and (policy.window_feats is not None) == (T > 1)
    assert torch.equal(env.obs, policy.env.obs)  # both leave env.obs on the state the last tick produced
