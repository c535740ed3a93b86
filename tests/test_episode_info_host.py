"""CPU-only checks of the per-episode info counters: the C ABI of ``susnet_episode_info`` against the header, the numpy path of ``EpisodeLog``
with an ``ep_info`` array against the reference train()'s own per-episode lists (tests/golden/episodes/epinfo_*.npz: what
``metrics.step(info)`` appended, train.py:419-427), and the shape of what ``train()`` puts into the metric handler / ``metrics.json``."""
import ctypes as C
import glob
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "episodes")
INFO_NAMES = ["imp_killed_crew", "imp_voted_out", "crew_voted_out", "sabotaged_jobs", "completed_jobs", "total_stalemates", "total_time_steps",
              "imposter_won", "crew_won"]  # SusMetrics order: the columns of the fixtures' `info` / `episode_info`


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def fixture_names():
    return sorted(os.path.basename(p)[len("epinfo_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "epinfo_*.npz")))


def load(pkg, name):
    d = np.load(os.path.join(GOLDEN, f"epinfo_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    assert meta["info_names"] == INFO_NAMES
    done, trunc, info = d["done"].astype(bool), d["trunc"].astype(bool), d["info"].astype(np.int64)
    roles = np.zeros(len(done), dtype=np.int64)
    for col in d["imposters"].T:
        roles |= 1 << col.astype(np.int64)
    c = {n: info[:, i] for i, n in enumerate(INFO_NAMES)}
    # every tick's info row as the record the stepping kernels write where an episode ends (the host path reads it at those ticks only)
    rec = pkg.episodes.pack_info(c["total_time_steps"], c["completed_jobs"], c["sabotaged_jobs"], c["imp_killed_crew"], c["imp_voted_out"],
                                 c["crew_voted_out"], c["imposter_won"], c["crew_won"])
    feed = {"rewards": d["reward"][:, None, :].copy(), "done": done[:, None].copy(), "truncated": trunc[:, None].copy(),
            "roles": roles.astype(np.int16)[:, None].copy(), "ep_info": rec[:, None].copy()}
    return {"meta": meta, "gamma": float(d["gamma"]), "feed": feed, "info": info, "episode_info": d["episode_info"].astype(np.int64),
            "imposter_return": d["avg_imposter_returns"], "crew_return": d["avg_crew_returns"]}


# ---- C ABI ----
def test_episode_info_structs_match_the_header(pkg, tmp_path):
    L = pkg._lib
    structs = {"susnet_episode_info": L.EpisodeInfo, "susnet_episode_io": L.EpisodeIO, "susnet_step_io": L.StepIO, "susnet_feed_io": L.FeedIO}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){"]
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ['printf("abi %d\\n", SUSNET_ABI_VERSION);', 'printf("crew_won %u\\n", SUSNET_OUTCOME_CREW_WON);',
              'printf("imposter_won %u\\n", SUSNET_OUTCOME_IMPOSTER_WON);', "return 0;}"]
    prog = tmp_path / "sizes.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, ct in structs.items():
        assert int(out[name]) == C.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(ct, fname).offset, f"{name}.{fname}"
    assert int(out["abi"]) == L.ABI_VERSION == 8
    assert (int(out["crew_won"]), int(out["imposter_won"])) == (L.OUTCOME_CREW_WON, L.OUTCOME_IMPOSTER_WON)
    # the new pointers sit at the END of the structs they were added to; the record is 16 bytes and the numpy dtype follows it
    assert L.StepIO._fields_[-1][0] == "ep_info" and L.FeedIO._fields_[-1][0] == "ep_info"
    assert [f for f, _ in L.EpisodeIO._fields_[-2:]] == ["info", "info_log"]
    dt = pkg.episodes.INFO_DTYPE
    assert dt.itemsize == C.sizeof(L.EpisodeInfo) == 16
    for fname, _ in L.EpisodeInfo._fields_:
        assert dt.fields[fname][1] == getattr(L.EpisodeInfo, fname).offset


def test_episode_stats_refuses_half_an_info_log(pkg):
    """Host-side validation only: no kernel is launched."""
    L = pkg._lib
    lib = L.lib()
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=200, n_imposters=1, n_crew=2, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                     shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    carry, ws = C.c_uint64(), C.c_uint64()
    assert lib.susnet_episode_stats_bytes(h, 5, C.byref(carry), C.byref(ws)) == 0
    io = L.EpisodeIO()
    io.n_ticks, io.gamma, io.capacity = 5, 0.9, 4
    io.rewards = io.done = io.truncated = io.roles = io.count = io.dropped = io.log = io.carry = io.workspace = 4096
    io.carry_bytes, io.workspace_bytes = carry.value, ws.value
    io.info = 4096
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"info" in lib.susnet_last_error()
    io.info, io.info_log = None, 4096
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"info" in lib.susnet_last_error()
    io.info, io.info_log = 4096 + 8, 4096
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"16-byte" in lib.susnet_last_error()
    sio = L.StepIO()
    sio.actions, sio.ep_info = 4096, 4096 + 4
    rc = lib.susnet_step(h, C.byref(sio), None)  # (refused before anything is launched: no state is bound either)
    assert rc in (L.E_INVALID, L.E_STATE)
    lib.susnet_destroy(h)


# ---- EpisodeLog, numpy path with ep_info ----
def test_info_fixture_set_is_not_vacuous(pkg):
    names = fixture_names()
    assert any(n.startswith("tagging") for n in names) and any(n.startswith("base_1v2") for n in names)
    total = np.zeros(9, dtype=np.int64)
    lengths = set()
    for n in names:
        f = load(pkg, n)
        ended = f["feed"]["done"][:, 0] | f["feed"]["truncated"][:, 0]
        assert len(f["episode_info"]) == ended.sum() >= 20 and not ended[-1], n
        total += f["episode_info"].sum(axis=0)
        lengths |= set(f["episode_info"][:, INFO_NAMES.index("total_time_steps")].tolist())
    for k in ("imp_killed_crew", "sabotaged_jobs", "completed_jobs", "total_time_steps", "imposter_won"):
        assert total[INFO_NAMES.index(k)] > 0, k
    assert total[INFO_NAMES.index("total_stalemates")] == 0 and len(lengths) > 5


@pytest.mark.parametrize("name", fixture_names())
@pytest.mark.parametrize("split", ["whole", "uneven"])
def test_numpy_path_reproduces_the_reference_info_lists(pkg, name, split):
    f = load(pkg, name)
    T = f["feed"]["rewards"].shape[0]
    log = pkg.EpisodeLog(gamma=f["gamma"], capacity=1024, n_agents=f["meta"]["n_agents"], batch=1)
    blocks, t, sizes = [], 0, (1, 5, 5, 3, 64, 7, 130, 2)
    while t < T:
        n = T - t if split == "whole" else min(sizes[len(blocks) % len(sizes)], T - t)
        blocks.append((t, t + n))
        t += n
    for t0, t1 in blocks:
        log.update({k: v[t0:t1] for k, v in f["feed"].items()})
    got = log.records()
    want = f["episode_info"]
    assert got["count"] == len(want) and got["dropped"] == 0
    for i, k in enumerate(INFO_NAMES):
        if k == "total_stalemates":
            continue
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[:, i]), k
    assert np.array_equal(got["total_time_steps"], got["length"])  # (the log starts with the run: no episode began before it)
    assert np.array_equal(got["imposter_return"].view(np.int64), f["imposter_return"].view(np.int64))
    assert np.array_equal(got["crew_return"].view(np.int64), f["crew_return"].view(np.int64))
    # ... and through the handler: the nine lists of the reference's metrics.json, which round-trips through load_metrics
    lists = pkg.train_loop.info_metric_lists(got)
    assert set(lists) == {pkg.SusMetrics(k) for k in INFO_NAMES}
    for i, k in enumerate(INFO_NAMES):
        assert lists[pkg.SusMetrics(k)] == want[:, i].tolist(), k


def test_numpy_path_info_log_overflow_and_word_view(pkg):
    f = load(pkg, fixture_names()[0])
    want = f["episode_info"]
    # the feed tensor's form: [T][B][4] int32 words
    words = f["feed"]["ep_info"].view(np.int32).reshape(-1, 1, 4)
    log = pkg.EpisodeLog(gamma=f["gamma"], capacity=5, n_agents=f["meta"]["n_agents"], batch=1)
    log.update(dict(f["feed"], ep_info=words))
    got = log.records()
    assert got["count"] == 5 and got["dropped"] == len(want) - 5
    assert np.array_equal(got["total_time_steps"], want[:5, INFO_NAMES.index("total_time_steps")])
    assert np.array_equal(got["completed_jobs"], want[:5, INFO_NAMES.index("completed_jobs")])
    # a log takes feeds with ep_info or without, not a mixture; a log without keeps returning what it returned before
    with pytest.raises(ValueError, match="ep_info"):
        log.update({k: v for k, v in f["feed"].items() if k != "ep_info"})
    plain = pkg.EpisodeLog(gamma=f["gamma"], capacity=8, n_agents=f["meta"]["n_agents"], batch=1)
    plain.update({k: v for k, v in f["feed"].items() if k != "ep_info"})
    assert "imposter_won" not in plain.records()
    with pytest.raises(ValueError, match="ep_info"):
        pkg.episodes.info_records(np.zeros((4, 1, 3), np.int32))


def test_pack_info_layout(pkg):
    rec = pkg.episodes.pack_info(np.array([7, 65535]), np.array([3, 1 << 20]), np.array([2, 0]), np.array([1, 300]), np.array([1, 0]),
                                 np.array([2, 15]), np.array([1, 0]), np.array([0, 1]))
    w = rec.view(np.uint32).reshape(2, 4)
    assert w[0].tolist() == [7, 3, 2, 1 | 1 << 8 | 2 << 16 | 2 << 24]
    assert w[1].tolist() == [65535, 1 << 20, 0, 255 | 0 << 8 | 15 << 16 | 1 << 24]  # (kills saturate at a byte)


# ---- train(): one entry per episode ----
class _FakeEnv:
    auto_reset, batch, n_agents, device = True, 1, 3, "cpu"

    def reset(self):
        pass


def test_train_fills_one_entry_per_episode(pkg, tmp_path):
    """``train()`` on a scripted feed (the fixture's ticks, block by block as the loop asks for them): the nine info entries of the handler
    have one value per episode, equal to a per-tick restatement of ``metrics.step(info)`` at every episode end; ``metrics.json`` has the
    reference's shape and round-trips through ``load_metrics``."""
    tl = pkg.train_loop
    f = load(pkg, [n for n in fixture_names() if n.startswith("base_1v2")][0])
    num_steps, k = 1200, 5
    env = _FakeEnv()

    class Ring:
        t = 0

        def collect(self, env_, policy, n, epsilon, ticks_per_append):
            assert n == ticks_per_append
            self.last_feed = ({key: v[self.t:self.t + n] for key, v in f["feed"].items()}, n)
            self.t += n

    class Policy:
        fused_imposter, fused_crew, crew_model = object(), None, None

    class Trainer:
        trained, gamma, models = (False, False), f["gamma"], (None, None)

        def sync_targets(self):
            pass

    Policy.env = Trainer.env = env
    metrics = pkg.EpisodicMetricHandler()
    log = pkg.EpisodeLog(gamma=f["gamma"], capacity=4096, n_agents=3, batch=1)
    tl.train(env, metrics, num_steps, Ring(), Policy(), Trainer(), pkg.ExponentialSchedule(1.0, 0.1, 100), tmp_path, train_step_interval=k,
             episode_log=log, per_episode_info=True)
    # the per-tick restatement: metrics.step(info) where done | truncated (train.py:419-427)
    want = pkg.EpisodicMetricHandler()
    for t in range(num_steps):
        if f["feed"]["done"][t, 0] or f["feed"]["truncated"][t, 0]:
            want.step({pkg.SusMetrics(n): int(f["info"][t, i]) for i, n in enumerate(INFO_NAMES)})
    n_ep = len(want.metrics[pkg.SusMetrics.TOTAL_TIME_STEPS])
    assert n_ep > 10
    for n in INFO_NAMES:
        got = metrics.metrics[pkg.SusMetrics(n)]
        assert len(got) == n_ep and got == want.metrics[pkg.SusMetrics(n)], n
    assert len(metrics.metrics[pkg.SusMetrics.AVG_IMPOSTER_RETURNS]) == n_ep
    means = metrics.compute()
    assert means[pkg.SusMetrics.TOTAL_TIME_STEPS] == sum(want.metrics[pkg.SusMetrics.TOTAL_TIME_STEPS]) / n_ep
    assert 0 < means[pkg.SusMetrics.IMPOSTER_WON] < 1 and means[pkg.SusMetrics.TOTAL_STALEMATES] == 0
    path = tmp_path / "metrics.json"
    metrics.save_metrics(path)
    back = pkg.EpisodicMetricHandler()
    back.load_metrics(path)
    for n in INFO_NAMES:
        assert back.metrics[n] == metrics.metrics[pkg.SusMetrics(n)] and len(back.metrics[n]) == n_ep
    # the first curve anybody plots: a moving average of imposter_won over episodes
    won = np.asarray(back.metrics["imposter_won"], dtype=np.float64)
    curve = np.convolve(won, np.ones(10) / 10, mode="valid")
    assert len(curve) == n_ep - 9 and curve.min() >= 0 and curve.max() <= 1
    # ... and the evaluation summary of the same log
    s = tl.summarize_episodes(log.records(), ticks=num_steps)
    assert s["episodes"] == n_ep and s["imposter_win_rate"] == won.mean() and s["mean_length"] == means[pkg.SusMetrics.TOTAL_TIME_STEPS]
    assert s["mean_completed_jobs"] == means[pkg.SusMetrics.COMPLETED_JOBS] and s["crew_win_rate"] == means[pkg.SusMetrics.CREW_WON]
