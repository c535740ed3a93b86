"""susnet_episode_stats (EpisodeLog's HIP path) on the MI355X: against the reference train()'s own episode records
(tests/golden/episodes/episodes_*.npz) bit for bit, many environments against the per-env host computation merged tick-major / env-minor,
log overflow, and hipGraph capture."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_fixtures as ef  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _env(pkg, meta, batch):
    """An env with the fixture's agent counts: the kernel reads (agents, batch) off its handle and nothing else."""
    kw = dict(batch=batch, device="cuda:0", rng="philox", seed=1, auto_reset=True)
    if meta["class"] == "itg":
        return pkg.BatchedImposterTrainingGround(n_crew=meta["n_crew"], n_jobs=0, time_step_reward=0, kill_reward=-3, sabotage_reward=0,
                                                 end_of_game_reward=0, grid=pkg.four_room_grid(9, False), **kw)
    return pkg.BatchedFourRoomEnv(meta["n_imposters"], meta["n_crew"], 2, **kw)


def _dev(feed):
    return {k: torch.as_tensor(v).to("cuda:0").contiguous() for k, v in feed.items()}


@pytest.mark.parametrize("name", ef.names())
@pytest.mark.parametrize("split", ["whole", "uneven"])
def test_kernel_reproduces_the_reference_bit_for_bit(pkg, name, split):
    f = ef.load(name)
    env = _env(pkg, f["meta"], 1)
    feed = _dev(f["feed"])
    T = feed["rewards"].shape[0]
    log = pkg.EpisodeLog(env, gamma=f["gamma"], capacity=256)
    for t0, t1 in ([(0, T)] if split == "whole" else ef.uneven_blocks(T)):
        log.update(ef.slice_feed(feed, t0, t1))
    got = log.records()
    ef.assert_records_equal(got, f)
    assert got["dropped"] == 0 and log.ticks == T


def _expected_merge(pkg, feed, gamma, A):
    """Per env by the numpy path (itself pinned to the reference on the CPU), merged tick-major, env-minor."""
    B = feed["rewards"].shape[1]
    rows = []
    for b in range(B):
        one = pkg.EpisodeLog(gamma=gamma, capacity=1 << 12, n_agents=A, batch=1)
        one.update({k: v[:, b:b + 1] for k, v in feed.items()})
        r = one.records()
        assert r["dropped"] == 0
        rows += [(int(r["tick"][i]), b, r["imposter_return"][i], r["crew_return"][i], int(r["length"][i]), int(r["ended_by"][i])) for i in range(r["count"])]
    rows.sort(key=lambda x: (x[0], x[1]))
    cols = list(zip(*rows))
    return {"tick": np.array(cols[0], np.int64), "env": np.array(cols[1], np.int32), "imposter_return": np.array(cols[2], np.float64),
            "crew_return": np.array(cols[3], np.float64), "length": np.array(cols[4], np.int32), "ended_by": np.array(cols[5], np.int32)}


@pytest.mark.parametrize("batch,family,ticks", [(200, "base14_1v2", 150), (4096, "base_3v9", 100), (4096, "itg_1v1", 100), (200, "base_1v10", 150),
                                                (4096, "base_2v6", 100)])
def test_many_envs_log_is_tick_major_env_minor_and_reproducible(pkg, batch, family, ticks):
    fx = [ef.load(n) for n in ef.names() if n.startswith(family)]
    assert len(fx) >= 2
    A, gamma = fx[0]["n_agents"], fx[0]["gamma"]
    host_feed = ef.merged_streams(fx, batch, ticks)
    want = _expected_merge(pkg, host_feed, gamma, A)
    assert len(want["tick"]) > batch // 8
    env = _env(pkg, fx[0]["meta"], batch)
    feed = _dev(host_feed)
    images = []
    for run in range(2):
        log = pkg.EpisodeLog(env, gamma=gamma, capacity=len(want["tick"]) + 64)
        for t0, t1 in ef.uneven_blocks(ticks, sizes=(1, 5, 5, 3, 64, 7)):
            log.update(ef.slice_feed(feed, t0, t1))
        got = log.records()
        ef.assert_records_equal(got, want)
        assert got["dropped"] == 0
        images.append((log._log.clone(), log._counters.clone(), log._carry.clone()))
    for a, b in zip(*images):
        assert torch.equal(a, b)
    # the carried state: G and t_episode of every env equal the host's after the same ticks
    host = pkg.EpisodeLog(gamma=gamma, capacity=len(want["tick"]), n_agents=A, batch=batch)
    host.update(host_feed)
    carry = images[0][2].cpu().numpy()
    G = carry[:2 * A * batch].view(np.float64).reshape(A, batch).T
    assert np.array_equal(G.view(np.int64), host._G.view(np.int64))
    assert np.array_equal(carry[2 * A * batch:], host._t_episode)


def test_log_overflow_counts_dropped_and_writes_nothing_past_the_log(pkg):
    L = pkg._lib
    fx = [ef.load(n) for n in ef.names() if n.startswith("base14_1v2")]
    B, T, A, gamma = 200, 120, 3, fx[0]["gamma"]
    host_feed = ef.merged_streams(fx, B, T)
    want = _expected_merge(pkg, host_feed, gamma, A)
    total = len(want["tick"])
    capacity, guard = total // 3, 64
    assert 0 < capacity < total
    env = _env(pkg, fx[0]["meta"], B)
    feed = _dev(host_feed)
    words = pkg.episodes.RECORD_DTYPE.itemsize // 8
    pattern = 0x5A5A5A5A5A5A5A5A
    buf = torch.full((capacity * words + guard,), pattern, dtype=torch.int64, device="cuda:0")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    cb, wb = C.c_uint64(), C.c_uint64()
    L.check(env.lib.susnet_episode_stats_bytes(env._h, 64, C.byref(cb), C.byref(wb)))
    carry = torch.zeros(cb.value // 4, dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(wb.value // 8 + 1, dtype=torch.int64, device="cuda:0")
    for t0, t1 in ef.uneven_blocks(T, sizes=(1, 5, 64, 3)):
        io = L.EpisodeIO()
        io.n_ticks = t1 - t0
        io.rewards, io.done = feed["rewards"][t0:t1].data_ptr(), feed["done"][t0:t1].data_ptr()
        io.truncated, io.roles = feed["truncated"][t0:t1].data_ptr(), feed["roles"][t0:t1].data_ptr()
        io.gamma, io.tick_base = gamma, t0
        io.carry, io.carry_bytes = carry.data_ptr(), carry.numel() * 4
        io.log, io.capacity = buf.data_ptr(), capacity
        io.count, io.dropped = counters.data_ptr(), counters.data_ptr() + 8
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        L.check(env.lib.susnet_episode_stats(env._h, C.byref(io), env._stream()))
    torch.cuda.synchronize()
    count, dropped = (int(v) for v in counters.cpu())
    assert count == capacity and dropped == total - capacity
    host = buf.cpu().numpy()
    assert (host[capacity * words:] == pattern).all(), "guard words after the log were written"
    rec = host[:capacity * words].view(pkg.episodes.RECORD_DTYPE)
    got = {k: rec[k] for k in ef.FIELDS}
    got["count"] = count
    ef.assert_records_equal(got, want, n=capacity)
    # the carried state advanced as if nothing had been dropped
    full = pkg.EpisodeLog(gamma=gamma, capacity=total, n_agents=A, batch=B)
    full.update(host_feed)
    c = carry.cpu().numpy()
    assert np.array_equal(c[:2 * A * B].view(np.float64).reshape(A, B).T.view(np.int64), full._G.view(np.int64))
    # a capacity of zero: everything is dropped, no log pointer is needed
    log0 = pkg.EpisodeLog(env, gamma=gamma, capacity=0)
    log0.update(feed)
    r0 = log0.records()
    assert r0["count"] == 0 and r0["dropped"] == total


def test_update_is_capturable_in_a_graph(pkg):
    fx = [ef.load(n) for n in ef.names() if n.startswith("base_2v6")]
    B, T, gamma = 1000, 60, fx[0]["gamma"]
    env = _env(pkg, fx[0]["meta"], B)
    feed = _dev(ef.merged_streams(fx, B, T))
    blocks = ef.uneven_blocks(T, sizes=(1, 5, 5, 3, 32))
    eager = pkg.EpisodeLog(env, gamma=gamma, capacity=1 << 14)
    for t0, t1 in blocks:
        eager.update(ef.slice_feed(feed, t0, t1))
    want = eager.records()
    assert want["count"] > 100
    log = pkg.EpisodeLog(env, gamma=gamma, capacity=1 << 14)
    log.update(ef.slice_feed(feed, 0, 32))  # warm-up: the workspace for the longest block
    torch.cuda.synchronize()
    log.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for t0, t1 in blocks:
                log.update(ef.slice_feed(feed, t0, t1))
    torch.cuda.current_stream().wait_stream(s)
    log.reset()
    graph.replay()
    torch.cuda.synchronize()
    got = log.records()
    ef.assert_records_equal(got, want)
    assert torch.equal(log._carry, eager._carry) and torch.equal(log._log, eager._log)


def test_unserved_agent_counts_are_refused(pkg):
    env = pkg.BatchedFourRoomEnv(4, 9, 2, batch=64, device="cuda:0", rng="philox", seed=1, auto_reset=True)  # 13 agents
    with pytest.raises(ValueError, match="agents"):
        pkg.EpisodeLog(env)
    cb, wb = C.c_uint64(), C.c_uint64()
    assert env.lib.susnet_episode_stats_bytes(env._h, 4, C.byref(cb), C.byref(wb)) == pkg._lib.E_INVALID
