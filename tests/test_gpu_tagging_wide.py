"""FourRoomEnvWithTagging with 9 .. 12 agents on the byte-parallel family kernels (three words of agent bytes: susnet_swar.h), on the GPU:
the reference fixtures of tests/golden/tagging_wide/ through the checks test_gpu_parity.py applies to the fixtures of tests/golden/,
a family sweep against the oracle, votes that reach quorum under random play, and the fused rollout against the drop-in API."""
import glob
import importlib
import os

import numpy as np
import pytest

import test_gpu_parity as tp
from conftest import GOLDEN_DIR, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDE_DIR = os.path.join(GOLDEN_DIR, "tagging_wide")
CRC_NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WIDE_DIR, "crc_*.npz")))
DIRECTED = "directed_tagging12_votes"
np_ = tp.np_


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("sus-net_amd")


def assert_in_family(pkg, meta, monkeypatch):
    """A handle of the fixture's game (made like the tests make theirs) selects a family instantiation: it has a packed record."""
    monkeypatch.delenv("SUSNET_FORCE_GENERIC", raising=False)
    env = tp.env_from_meta(pkg, meta, 4, rng="numpy", tape_words=1 << 10)
    assert env.record_layout() is not None, "tagging games with 9 .. 12 agents run the byte-parallel family kernels"
    del env


# ------------------------------------------------------------------------------------------------
# the reference fixtures
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", tp.KERNELS)
def test_hip_replays_the_directed_twelve_agent_votes(pkg, kernels, monkeypatch):
    """test_gpu_parity.test_hip_replays_reference_traces on the directed 12-agent fixture, through rng="numpy" handles with the recorded seed
    and injections: state, reward bit patterns, flags, the 13 counters, used / counts / timer after every step and the words consumed --
    once through k_step of the family instantiation, once through the generic kernel (SUSNET_FORCE_GENERIC=1)."""
    g = load_golden(os.path.join(WIDE_DIR, DIRECTED + ".npz"))
    assert g["meta"]["n_agents"] == 12
    if kernels == "compiled":
        assert_in_family(pkg, g["meta"], monkeypatch)
    monkeypatch.setattr(tp, "GOLDEN_DIR", WIDE_DIR)
    monkeypatch.setattr(tp, "FAMILIES", {DIRECTED: [DIRECTED]})
    tp.test_hip_replays_reference_traces(pkg, DIRECTED, kernels, monkeypatch)


@pytest.mark.parametrize("name", CRC_NAMES)
def test_hip_matches_the_wide_tagging_crc_streams(pkg, name, monkeypatch):
    """64 numpy seeds x 96 steps through the step API of the family instantiation (test_gpu_parity.test_hip_matches_reference_crc_streams)."""
    assert_in_family(pkg, load_golden(os.path.join(WIDE_DIR, name + ".npz"))["meta"], monkeypatch)
    monkeypatch.setattr(tp, "GOLDEN_DIR", WIDE_DIR)
    tp.test_hip_matches_reference_crc_streams(pkg, name, "compiled", monkeypatch)


@pytest.mark.parametrize("epw", [16, 64])
@pytest.mark.parametrize("layout", ["separate", "packed"])
@pytest.mark.parametrize("name", CRC_NAMES)
def test_fused_rollout_on_numpy_tapes_matches_the_wide_tagging_crc_streams(pkg, oracle_mod, name, layout, epw, monkeypatch):
    """... and through ONE launch of the fused rollout fed numpy's words (k_rollout_swar<*, OUT_TRAJ_RAW8 / OUT_RECORD, TapeRng>; the shuffle of
    the action order stays rolled there), a partly and a fully used wave: test_gpu_parity.test_fused_rollout_on_numpy_tapes_matches_reference_crc_streams."""
    assert_in_family(pkg, load_golden(os.path.join(WIDE_DIR, name + ".npz"))["meta"], monkeypatch)
    monkeypatch.setattr(tp, "GOLDEN_DIR", WIDE_DIR)
    tp.test_fused_rollout_on_numpy_tapes_matches_reference_crc_streams(pkg, oracle_mod, name, layout, epw, monkeypatch)


# ------------------------------------------------------------------------------------------------
# against the oracle on the production (Philox) stream
# ------------------------------------------------------------------------------------------------
def compare_rollout(env, ob, traj, T, tag):
    acts, rews, dones, truncs, obs = (np_(traj[k]) for k in ("actions", "rewards", "done", "truncated", "obs"))
    for s in range(T):
        oa = ob.sample_actions()
        assert np.array_equal(acts[s], oa), f"{tag} actions tick {s}"
        orew, odone, otrunc, rc = ob.step(oa)
        assert rc == 0
        assert np.array_equal(rews[s].astype(np.float64).view(np.uint64), orew.view(np.uint64)), f"{tag} rewards tick {s}"
        assert np.array_equal(dones[s], odone.astype(bool)) and np.array_equal(truncs[s], otrunc.astype(bool)), f"{tag} flags tick {s}"
        ob.reset(mask=(odone | otrunc).astype(bool))
        assert np.array_equal(obs[s], ob.obs_raw_u8()), f"{tag} raw obs tick {s}"


@pytest.mark.parametrize("n_imp", [1, 2, 3])
@pytest.mark.parametrize("A", [9, 10, 11, 12])
def test_wide_tagging_family_sweep_matches_oracle(pkg, oracle_mod, A, n_imp):
    """The tagging instantiations with three words of agent bytes (the cases test_gpu_parity.test_family_sweep_matches_oracle skips): no jobs and
    five, both action orders, fixed and shuffled roles, a ragged last wave, 12-step episodes, votes every five steps -- packed records AND
    separate tensors with the raw observation, then 8 steps of the drop-in API on the same handle, then the whole state."""
    B, T, n_cases = 64 * 2 + 3, 36, 0
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    for J in (0, 5):
        for order_random in (True, False):
            for shuffle in (False, True):
                kw = dict(n_imposters=n_imp, n_crew=A - n_imp, n_jobs=J, max_time_steps=12, shuffle_imposter_index=shuffle, is_action_order_random=order_random,
                          tag_reset_interval=5)
                name = f"wide sweep tagging {n_imp}v{A - n_imp} j{J} order{int(order_random)} shuffle{int(shuffle)}"
                tp.CONFIGS[name] = dict(cls="tagging", kw=kw, n=9)
                try:
                    for packed in (True, False):
                        env, ob = tp.make_pair(pkg, oracle_mod, name, B, 40 + J, auto_reset=True, check_errors=False)
                        assert env.record_layout() is not None, f"{name}: every 3..12-agent game with at most 3 imposters and 8 jobs is in the family"
                        env.reset()
                        ob.reset()
                        traj = env.rollout(T, obs=raw8, packed=packed)
                        torch.cuda.synchronize()
                        compare_rollout(env, ob, traj, T, f"{name} packed={packed}")
                        if not packed:  # ... then the drop-in API on the same handle (k_sample_philox + k_step of the same instantiation)
                            for s_ in range(8):
                                a = env.sample_actions().clone()
                                oa = ob.sample_actions()
                                assert np.array_equal(np_(a), oa), f"{name} api actions step {s_}"
                                _, rew, done, trunc, _ = env.step(a)
                                orew, odone, otrunc, _ = ob.step(oa)
                                assert np.array_equal(np_(rew).astype(np.float64).view(np.uint64), orew.view(np.uint64)), f"{name} api rewards step {s_}"
                                assert np.array_equal(np_(done), odone.astype(bool)) and np.array_equal(np_(trunc), otrunc.astype(bool))
                                ob.reset(mask=(odone | otrunc).astype(bool))
                        env._export(full=True)
                        tp.compare_full_state(env, ob, f"{name} packed={packed}")
                        n_cases += 1
                        del env, ob, traj
                finally:
                    del tp.CONFIGS[name]
    assert n_cases == 16


@pytest.mark.parametrize("A", [9, 12])
def test_votes_reach_quorum_under_random_play(pkg, oracle_mod, A):
    """With nine or more living agents random tags almost never reach quorum, so the sweep above does not test the vote.  Here every vote interval
    starts from an imported state with three agents alive -- the imposter (agent 0), agent 5 and the highest index; quorum 2 -- while the dead
    keep tagging (tagging.py:103-110 never checks the actor): 8 intervals of 5 ticks through the fused rollout, packed records and separate
    tensors in turn, everything bit-exact against the oracle.
    Condition (the oracle's own counters, asserted before anything is compared): at least 10 ejections over the batch, at least one of an agent
    of index >= 8.  The oracle alone gives, for seed 77 and B = 131: A = 9: 1019 ejections, 257 of agent 8; A = 12: 1032 ejections, 283 of agent 11
    (counted where no kill landed in the same step, so that the agent that died is the ejected one)."""
    B, interval, n_intervals, seed = 64 * 2 + 3, 5, 8, 77
    name = f"wide votes tagging 1v{A - 1}"
    kw = dict(n_imposters=1, n_crew=A - 1, n_jobs=2, shuffle_imposter_index=False, tag_reset_interval=interval)
    alive = np.zeros((B, A), dtype=np.uint8)
    alive[:, [0, 5, A - 1]] = 1
    zeros = np.zeros((B, A), dtype=np.int32)

    def import_state(env, ob):
        if env is not None:
            env.set_state(alive_agents=alive, used_tag_actions=zeros, tag_counts=zeros, tag_reset_timer=zeros[:, 0], t=zeros[:, 0])
        for b in range(B):
            ob.set_state(b, alive=alive[b], used=zeros[b], counts=zeros[b], timer=0, t=0)

    def oracle_ejections():
        """(ejections, ejections of an agent of index >= 8) of the oracle's own run of the test's schedule"""
        ob = oracle_mod.OracleBatch(oracle_mod.make_config("tagging", grid=pkg.four_room_grid(9, True).astype(np.uint8), **kw), B)
        ob.set_philox(seed, 0, 0)
        ob.reset()
        total = high = 0
        for _ in range(n_intervals):
            import_state(None, ob)
            for _ in range(interval):
                before = ob.export()
                _, odone, otrunc, rc = ob.step(ob.sample_actions())
                assert rc == 0
                after = ob.export()
                voted = (after["metrics"][:, 1:3].sum(axis=1) - before["metrics"][:, 1:3].sum(axis=1)) > 0
                killed = (after["metrics"][:, 0] - before["metrics"][:, 0]) > 0
                died_high = ((before["alive"][:, 8:] == 1) & (after["alive"][:, 8:] == 0)).any(axis=1)
                total += int(voted.sum())
                high += int((voted & ~killed & died_high).sum())  # (no kill in the same step: the agent that died is the ejected one)
                ob.reset(mask=(odone | otrunc).astype(bool))
        return total, high

    total, high = oracle_ejections()
    print(f"{name}: the oracle ejects {total} agents over the batch, {high} of them of index >= 8")
    assert total >= 10 and high >= 1, (total, high)

    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    tp.CONFIGS[name] = dict(cls="tagging", kw=kw, n=9)
    try:
        env, ob = tp.make_pair(pkg, oracle_mod, name, B, seed, auto_reset=True, check_errors=False)
    finally:
        del tp.CONFIGS[name]
    assert env.record_layout() is not None
    env.reset()
    ob.reset()
    for k in range(n_intervals):
        import_state(env, ob)
        packed = k % 2 == 0
        traj = env.rollout(interval, obs=raw8, packed=packed)
        torch.cuda.synchronize()
        compare_rollout(env, ob, traj, interval, f"{name} interval {k} packed={packed}")
    env._export(full=True)
    tp.compare_full_state(env, ob, name)


def test_fused_rollout_equals_the_drop_in_api_on_a_twin_handle(pkg):
    """tagging 3v9 j8 (12 agents, shuffled roles, a shuffled action order: six action-stream words per tick) at B = 4096 for 64 ticks: the fused
    rollout (k_rollout_swar) against sample_actions() / step() tick by tick (k_sample_philox + k_step) on a twin handle -- identical actions,
    rewards, flags and final state; it ties the two kernels of an instantiation together."""
    B, T, seed = 4096, 64, 5
    kw = dict(n_imposters=3, n_crew=9, n_jobs=8, tag_reset_interval=4, max_time_steps=40, batch=B, rng="philox", seed=seed, auto_reset=True,
              check_errors=False, grid=pkg.four_room_grid(9, True))
    fused, twin = pkg.BatchedFourRoomEnvWithTagging(**kw), pkg.BatchedFourRoomEnvWithTagging(**kw)
    assert fused.record_layout() is not None
    fused.reset()
    twin.reset()
    traj = fused.rollout(T, obs=pkg.ObsConfig("raw", dtype=torch.uint8), packed=False)
    torch.cuda.synchronize()
    n_done = 0
    for s in range(T):
        a = twin.sample_actions().clone()
        assert torch.equal(traj["actions"][s].to(a.dtype), a), f"actions tick {s}"
        _, rew, done, trunc, _ = twin.step(a)
        assert torch.equal(traj["rewards"][s].view(torch.int32), rew.to(torch.float32).view(torch.int32)), f"rewards tick {s}"
        assert torch.equal(traj["done"][s].bool(), done.bool()) and torch.equal(traj["truncated"][s].bool(), trunc.bool()), f"flags tick {s}"
        n_done += int(done.sum())
    assert n_done > 0
    fused._export(full=True)
    twin._export(full=True)
    for field in ("agent_positions", "alive_agents", "imposter_mask", "job_positions", "completed_jobs", "t", "used_tag_actions", "tag_counts", "_timer"):
        assert torch.equal(getattr(fused, field), getattr(twin, field)), field
    assert torch.equal(fused.rng_cursor(), twin.rng_cursor()) and torch.equal(fused.episode_index(), twin.episode_index())
    twin.poll_errors()
    fused.poll_errors()
