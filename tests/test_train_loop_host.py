"""CPU-only checks of the device training loop's host side: the epsilon schedule, the block planner against a per-tick restatement of the
reference's loop order (src/train.py:328-416), the numpy path of ``EpisodeLog`` against the reference train()'s own episode records
(tests/golden/episodes/episodes_*.npz, bit for bit), and the C ABI of ``susnet_episode_stats``."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_fixtures as ef  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


# ---- ExponentialSchedule (src/scheduler.py) ----
def test_exponential_schedule_closed_form(pkg):
    v0, v1, n = 1.0, 0.05, 1_000_000  # run_experiment's defaults (train.py:165-167)
    s = pkg.ExponentialSchedule(v0, v1, n)
    b = math.log(v1 / v0) / (n - 1)
    assert s.value(-1) == v0 and s.value(0) == v0
    for step in (1, n // 2, n - 1):
        assert s.value(step) == pytest.approx(v0 * math.exp(b * step), rel=1e-15)
    assert s.value(1) < v0 and s.value(n - 1) == pytest.approx(v1, rel=1e-12)
    assert s.value(n) == v1 and s.value(10 * n) == v1
    small = pkg.ExponentialSchedule(0.9, 0.1, 11)
    assert [small.value(t) for t in range(1, 10)] == sorted((small.value(t) for t in range(1, 10)), reverse=True)


# ---- the block planner against the reference's per-tick order ----
def _reference_order(num_steps, k, u, num_saves):
    """train.py:328-416 tick by tick: save (name, weights version), target sync, [act, step, add], train.  -> (train ticks, per train step
    the sync ticks since the previous one and the weights version the targets hold, saves)."""
    t_saves = np.linspace(0, num_steps, num_saves - 1, endpoint=False, dtype=int)
    version, target, pending = 0, None, []
    train_ticks, per_train, saves = [], [], []
    for t in range(num_steps):
        if t in t_saves:
            saves.append((f"imposter_mlp_{int(t * 100 / num_steps)}.pt", version))
        if t % u == 0:
            target = version
            pending.append(t)
        if t % k == 0:
            train_ticks.append(t)
            per_train.append((tuple(pending), target))
            pending = []
            version += 1
    return train_ticks, per_train, saves, tuple(pending)


def _planned_order(pkg, num_steps, k, u, num_saves):
    tl = pkg.train_loop
    model = pkg.MLP([4, 8, 8, 8, 8, 3])
    version, target, pending = 0, None, []
    train_ticks, per_train, saves = [], [], []
    t_next = 0
    for blk in tl.plan_blocks(num_steps, k, u, num_saves):
        assert blk.t0 == t_next and blk.n_ticks >= 1
        t_next = blk.t0 + blk.n_ticks
        assert all(blk.t0 <= t < t_next for t in blk.sync_ticks + blk.save_ticks)
        for t in blk.save_ticks:
            saves.append((tl.checkpoint_name("imposter", model, int(t * 100 / num_steps)), version))
        if blk.sync_ticks:
            target = version
            pending += list(blk.sync_ticks)
        if blk.trains:
            train_ticks.append(t_next - 1)
            per_train.append((tuple(pending), target))
            pending = []
            version += 1
    assert t_next == num_steps
    return train_ticks, per_train, saves, tuple(pending)


@pytest.mark.parametrize("num_steps", [1, 2, 3, 7, 40, 41, 100, 257])
@pytest.mark.parametrize("k", [1, 3, 5, 64, 300])
@pytest.mark.parametrize("u", [1, 4, 7, 10_000])
@pytest.mark.parametrize("num_saves", [1, 2, 5, 9])
def test_block_plan_equals_the_per_tick_order(pkg, num_steps, k, u, num_saves):
    assert _planned_order(pkg, num_steps, k, u, num_saves) == _reference_order(num_steps, k, u, num_saves)
    blocks = pkg.plan_blocks(num_steps, k, u, num_saves)
    assert blocks[0].n_ticks == 1 and all(b.n_ticks <= k for b in blocks)
    assert all(b.n_ticks == k for b in blocks[1:-1])


def test_checkpoint_names(pkg):
    tl = pkg.train_loop
    assert tl.checkpoint_name("imposter", pkg.MLP([4, 8, 8, 8, 8, 3]), 25) == "imposter_mlp_25.pt"
    assert tl.checkpoint_name("crew", pkg.MLP([4, 8, 8, 8, 8, 3]), "100%") == "crew_mlp_100%.pt"
    assert tl.model_type(pkg.RandomEquiprobable(3)) == "random" and tl.model_type(None) == "random"


# ---- EpisodeLog, numpy path ----
def test_numpy_order_mean_is_numpys_mean(pkg):
    rng = np.random.default_rng(5)
    for n in range(1, 13):
        for _ in range(300):
            x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
            full = np.zeros(16)
            where = np.sort(rng.choice(16, n, replace=False))
            full[where] = x
            mask = np.zeros(16, bool)
            mask[where] = True
            assert pkg.episodes.numpy_order_mean(x) == full[mask].mean().item() == x.mean().item()
    assert math.isnan(pkg.episodes.numpy_order_mean([]))


def test_fixture_set_is_not_vacuous():
    fx = [ef.load(n) for n in ef.names()]
    assert len(fx) >= 8 and len({f["gamma"] for f in fx}) >= 2 and all(f["gamma"] < 1 for f in fx)
    assert {f["n_agents"] for f in fx} >= {2, 3, 8} and any(f["meta"]["n_crew"] >= 8 for f in fx)
    for f in fx:
        ended = f["feed"]["done"][:, 0] | f["feed"]["truncated"][:, 0]
        assert len(f["tick"]) >= 20 and not ended[-1], f["name"]
        r = f["feed"]["rewards"].astype(np.float64)
        assert np.array_equal(r * 4, np.round(r * 4)), "rewards are multiples of 0.25: exact in float32"
    assert any((f["ended_by"] == 2).sum() >= 5 for f in fx) and any((f["ended_by"] & 1).sum() >= 5 for f in fx)


@pytest.mark.parametrize("name", ef.names())
@pytest.mark.parametrize("split", ["whole", "uneven"])
def test_numpy_path_reproduces_the_reference_bit_for_bit(pkg, name, split):
    f = ef.load(name)
    T = f["feed"]["rewards"].shape[0]
    log = pkg.EpisodeLog(gamma=f["gamma"], capacity=1024, n_agents=f["n_agents"], batch=1)
    for t0, t1 in ([(0, T)] if split == "whole" else ef.uneven_blocks(T)):
        log.update(ef.slice_feed(f["feed"], t0, t1))
    got = log.records()
    ef.assert_records_equal(got, f)
    assert got["dropped"] == 0 and log.ticks == T


def test_numpy_path_many_envs_is_the_tick_major_merge(pkg):
    fx = [ef.load(n) for n in ef.names() if n.startswith("base14_1v2")]
    B, T = 7, 150
    feed = ef.merged_streams(fx, B, T)
    log = pkg.EpisodeLog(gamma=0.9, capacity=4096, n_agents=3, batch=B)
    for t0, t1 in ef.uneven_blocks(T):
        log.update(ef.slice_feed(feed, t0, t1))
    got = log.records()
    rows = []
    for b in range(B):
        one = pkg.EpisodeLog(gamma=0.9, capacity=4096, n_agents=3, batch=1)
        one.update({k: v[:, b:b + 1] for k, v in feed.items()})
        r = one.records()
        rows += [(int(r["tick"][i]), b, r["imposter_return"][i], r["crew_return"][i], int(r["length"][i]), int(r["ended_by"][i])) for i in range(r["count"])]
    rows.sort(key=lambda x: (x[0], x[1]))
    want = {"tick": [r[0] for r in rows], "env": [r[1] for r in rows], "imposter_return": [r[2] for r in rows], "crew_return": [r[3] for r in rows],
            "length": [r[4] for r in rows], "ended_by": [r[5] for r in rows]}
    assert len(rows) > 20
    ef.assert_records_equal(got, {k: np.asarray(v) for k, v in want.items()})


def test_numpy_path_overflow_counts_dropped(pkg):
    f = ef.load(ef.names()[0])
    log = pkg.EpisodeLog(gamma=f["gamma"], capacity=5, n_agents=f["n_agents"], batch=1)
    log.update(f["feed"])
    got = log.records()
    ef.assert_records_equal(got, f, n=5)
    assert got["dropped"] == len(f["tick"]) - 5
    log.reset()
    assert log.records()["count"] == 0 and log.ticks == 0


# ---- C ABI ----
def test_episode_structs_match_the_header(pkg, tmp_path):
    L = pkg._lib
    structs = {"susnet_episode_record": L.EpisodeRecord, "susnet_episode_io": L.EpisodeIO}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){"]
    for name, ct in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ['printf("abi %d\\n", SUSNET_ABI_VERSION);', 'printf("done %d\\n", SUSNET_EPISODE_DONE);',
              'printf("truncated %d\\n", SUSNET_EPISODE_TRUNCATED);', "return 0;}"]
    prog = tmp_path / "sizes.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, ct in structs.items():
        assert int(out[name]) == C.sizeof(ct), name
        for fname, _ in ct._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(ct, fname).offset, f"{name}.{fname}"
    assert int(out["abi"]) == L.ABI_VERSION >= 7
    assert (int(out["done"]), int(out["truncated"])) == (L.EPISODE_DONE, L.EPISODE_TRUNCATED)
    assert pkg.episodes.RECORD_DTYPE.itemsize == C.sizeof(L.EpisodeRecord) == 40
    for fname, _ in L.EpisodeRecord._fields_:
        assert pkg.episodes.RECORD_DTYPE.fields[fname][1] == getattr(L.EpisodeRecord, fname).offset


def test_episode_symbols_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    for name in ("susnet_episode_stats", "susnet_episode_stats_bytes"):
        assert name in declared and name in pkg._lib.EXPORTS and hasattr(lib, name)


def _handle(L, lib, **kw):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    d = dict(variant=L.VARIANT_BASE, batch=200, n_imposters=1, n_crew=2, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
             shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX)
    d.update(kw)
    for k, v in d.items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


def test_episode_stats_sizes_and_argument_checks(pkg):
    """Host-side validation only: no kernel is launched (every call below is refused, or only computes sizes)."""
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)
    carry, ws = C.c_uint64(), C.c_uint64()
    assert lib.susnet_episode_stats_bytes(h, 5, C.byref(carry), C.byref(ws)) == 0
    assert carry.value == 200 * (3 * 8 + 4)  # float64 G[A][B], int32 t_episode[B]
    W = (200 + 63) // 64
    assert ws.value >= 5 * W * (4 + 8)  # a count and a position per (tick, wave)
    ws1 = C.c_uint64()
    assert lib.susnet_episode_stats_bytes(h, 500, C.byref(carry), C.byref(ws1)) == 0 and ws1.value > ws.value
    assert lib.susnet_episode_stats_bytes(h, 0, C.byref(carry), C.byref(ws)) == L.E_INVALID
    assert lib.susnet_episode_stats_bytes(h, 5, None, C.byref(ws)) == L.E_INVALID
    assert lib.susnet_episode_stats_bytes(None, 5, C.byref(carry), C.byref(ws)) == L.E_INVALID
    io = L.EpisodeIO()
    io.n_ticks = 5
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"null" in lib.susnet_last_error()
    assert lib.susnet_episode_stats(h, None, None) == L.E_INVALID
    io.rewards = io.done = io.truncated = io.roles = io.count = io.dropped = 4096
    io.capacity = 4
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"log" in lib.susnet_last_error()
    io.log = 4096
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"carry" in lib.susnet_last_error()
    io.carry, io.carry_bytes = 4096, carry.value - 1
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"carry" in lib.susnet_last_error()
    io.carry_bytes = carry.value
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"workspace" in lib.susnet_last_error()
    io.workspace, io.workspace_bytes, io.n_ticks = 4096, ws1.value, 0
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"n_ticks" in lib.susnet_last_error()
    io.n_ticks, io.gamma = 5, float("nan")
    assert lib.susnet_episode_stats(h, C.byref(io), None) == L.E_INVALID and b"gamma" in lib.susnet_last_error()
    lib.susnet_destroy(h)


def test_episode_log_argument_checks(pkg):
    with pytest.raises(ValueError, match="agents"):
        pkg.EpisodeLog(n_agents=13, batch=1)
    with pytest.raises(ValueError, match="needs the env"):
        pkg.EpisodeLog(n_agents=3, batch=1, device="cuda:0")
    log = pkg.EpisodeLog(n_agents=3, batch=2)
    feed = {"rewards": np.zeros((4, 2, 3), np.float32), "done": np.zeros((4, 2), bool), "truncated": np.zeros((4, 2), bool),
            "roles": np.ones((4, 2), np.int16)}
    with pytest.raises(ValueError, match="n_ticks"):
        log.update(feed, n_ticks=5)
    with pytest.raises(ValueError, match="rewards"):
        log.update(dict(feed, rewards=np.zeros((4, 3, 3), np.float32)))
    log.update(feed, n_ticks=3)
    assert log.ticks == 3 and log.records()["count"] == 0
