"""CPU-only checks of resumable runs: where ``stop_after`` / ``snapshot_interval`` fall on a block plan, ``state_dict`` -> fresh object ->
``load_state_dict`` of the CPU ring and the CPU ``EpisodeLog`` (a ring that has wrapped; both objects continued with the same further
input), the refusals of a resume (config comparison, missing file, another ABI version, a finished run's file) and the atomic write of
``run_state.pt``."""
import importlib
import inspect
import io
import json

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def _through_a_file(sd):
    """What a snapshot goes through: torch.save, then the restricted loader ``read_run_state`` uses."""
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)


# ---- stop_after / snapshot_interval -> block boundaries ----
def _boundaries(blocks):
    return [b.t0 + b.n_ticks for b in blocks]


def test_block_boundaries_are_one_then_every_k(pkg):
    assert _boundaries(pkg.plan_blocks(41, 5, 10, 5)) == [1, 6, 11, 16, 21, 26, 31, 36, 41]
    assert _boundaries(pkg.plan_blocks(7, 1, 10, 5)) == [1, 2, 3, 4, 5, 6, 7]
    assert _boundaries(pkg.plan_blocks(13, 5, 10, 5)) == [1, 6, 11, 13]  # (a shorter last block that ends with the run)


@pytest.mark.parametrize("num_steps, k, cases", [
    (41, 5, {-3: 1, 0: 1, 1: 1, 2: 6, 6: 6, 7: 11, 16: 16, 17: 21, 40: 41, 41: 41, 42: None, 1000: None}),
    (7, 1, {0: 1, 1: 1, 2: 2, 5: 5, 7: 7, 8: None}),
    (13, 5, {11: 11, 12: 13, 13: 13, 14: None}),
])
def test_stop_boundary(pkg, num_steps, k, cases):
    blocks = pkg.plan_blocks(num_steps, k, 10, 5)
    for t, want in cases.items():
        got = pkg.stop_boundary(blocks, t)
        assert got == want, (t, got, want)
        if got is not None:  # the first boundary with at least t completed ticks
            assert got >= t and got in _boundaries(blocks) and not any(t <= b < got for b in _boundaries(blocks))


def test_snapshot_boundaries(pkg):
    blocks = pkg.plan_blocks(41, 5, 10, 5)
    assert pkg.snapshot_boundaries(blocks, 10) == [11, 21, 31]  # (41 is the run's end: it finishes there instead)
    assert pkg.snapshot_boundaries(blocks, 1) == [1, 6, 11, 16, 21, 26, 31, 36]
    assert pkg.snapshot_boundaries(blocks, 12) == [16, 26, 36]  # due at 12, 24 (first multiple past 16), 36
    assert pkg.snapshot_boundaries(blocks, 100) == []
    assert pkg.snapshot_boundaries(pkg.plan_blocks(7, 1, 10, 5), 3) == [3, 6]
    with pytest.raises(ValueError, match="snapshot_interval"):
        pkg.snapshot_boundaries(blocks, 0)
    # a resumed run names the same boundaries: the function reads the plan alone
    assert [b for b in pkg.snapshot_boundaries(blocks, 10) if b > 16] == [21, 31]


def test_the_entry_points_take_the_three_arguments_with_default_none(pkg):
    for fn in (pkg.run_experiment, pkg.run_sweep, pkg.train, pkg.train_sweep):
        params = inspect.signature(fn).parameters
        for name in ("snapshot_interval", "stop_after", "resume_from"):
            assert name in params and params[name].default is None, (fn.__name__, name)


# ---- the CPU ring ----
RING = dict(max_size=20, state_size=6, trajectory_size=2, n_agents=3, n_imposters=1)
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")


def _rows(g, n):
    T, S, A = RING["trajectory_size"], RING["state_size"], RING["n_agents"]
    return (torch.randint(0, 9, (n, T, S), generator=g).float(), torch.randint(0, 8, (n, A), generator=g),
            torch.randn(n, A, generator=g), torch.randint(0, 9, (n, T, S), generator=g).float(), torch.rand(n, generator=g) < 0.3,
            torch.randint(0, A, (n, 1), generator=g))


@pytest.mark.parametrize("adds", [2, 4])  # 14 rows: not full, rows 0 .. 13 saved; 28 rows: the ring of 20 has wrapped once
def test_ring_state_dict_roundtrip_and_continuation(pkg, adds):
    g = torch.Generator().manual_seed(11)
    ring = pkg.DeviceReplayBuffer(**RING, device="cpu")
    for _ in range(adds):
        ring.add_batch(*_rows(g, 7))
    assert (ring.size, ring.idx) == ((14, 14) if adds == 2 else (20, 8))
    sd = _through_a_file(ring.state_dict())
    assert sd["rows"]["states"].shape[0] == ring.size and sd["collect_window"] is None
    fresh = pkg.DeviceReplayBuffer(**RING, device="cpu")
    for f in RING_FIELDS:  # anything left unrestored shows
        getattr(fresh, f).fill_(1)
    fresh.load_state_dict(sd)
    assert (fresh.idx, fresh.size) == (ring.idx, ring.size)
    more = [_rows(g, 7), _rows(g, 5)]
    for r in (ring, fresh):
        for rows in more:
            r.add_batch(*rows)
    assert (fresh.idx, fresh.size) == (ring.idx, ring.size) == ((14 + 12) % 20 if adds == 2 else (8 + 12) % 20, 20)
    for f in RING_FIELDS:
        assert torch.equal(getattr(fresh, f), getattr(ring, f)), f
    torch.manual_seed(3)
    a = ring.sample(16)
    torch.manual_seed(3)
    b = fresh.sample(16)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_ring_refuses_another_shape(pkg):
    sd = pkg.DeviceReplayBuffer(**RING, device="cpu").state_dict()
    with pytest.raises(ValueError, match="trajectory_size = 2, this one has 3"):
        pkg.DeviceReplayBuffer(**dict(RING, trajectory_size=3), device="cpu").load_state_dict(sd)


# ---- the CPU EpisodeLog ----
def _feed(rng, T, B, A, with_info):
    ep = pkg_episodes()
    done = rng.random((T, B)) < 0.25
    trunc = ~done & (rng.random((T, B)) < 0.15)
    feed = {"rewards": rng.integers(-3, 4, (T, B, A)).astype(np.float32), "done": done, "truncated": trunc,
            "roles": (1 << rng.integers(0, A, (T, B))).astype(np.int16)}
    if with_info:
        n = rng.integers(0, 40, (6, T, B))
        feed["ep_info"] = ep.pack_info(n[0], n[1], n[2], n[3] % 4, n[4] % 2, n[5] % 3, done & (n[0] % 2 == 0), done & (n[0] % 2 == 1))
    return feed


def pkg_episodes():
    return importlib.import_module("sus-net_amd").episodes


@pytest.mark.parametrize("with_info", [False, True])
def test_cpu_episode_log_state_dict_roundtrip_and_continuation(pkg, with_info):
    rng = np.random.default_rng(5)
    A, B = 3, 4
    log = pkg.EpisodeLog(n_agents=A, batch=B, gamma=0.9, capacity=20)  # (small: the later feeds find it full, `dropped` counts)
    for T in (3, 5):
        log.update(_feed(rng, T, B, A, with_info), tick_base=None)
    before = log.records()
    assert 0 < before["count"] < 20 and (log._G != 0).any() and (log._t_episode != 0).any()  # episodes in flight at the cut
    sd = _through_a_file(log.state_dict())
    fresh = pkg.EpisodeLog(n_agents=A, batch=B, gamma=0.9, capacity=20)
    fresh.load_state_dict(sd)
    assert fresh.ticks == log.ticks == 8 and fresh.has_info is with_info
    more = [_feed(rng, 5, B, A, with_info), _feed(rng, 4, B, A, with_info)]
    for l in (log, fresh):
        for feed in more:
            l.update(feed)
    a, b = log.records(), fresh.records()
    assert a.keys() == b.keys() and a["count"] == b["count"] == 20 and a["dropped"] == b["dropped"] > 0
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert np.array_equal(log._G.view(np.uint64), fresh._G.view(np.uint64)) and np.array_equal(log._t_episode, fresh._t_episode)
    assert np.array_equal(log._host_log, fresh._host_log) and fresh.ticks == log.ticks == 17
    if with_info:
        assert np.array_equal(log._info_log, fresh._info_log)


def test_cpu_episode_log_refuses_another_shape(pkg):
    sd = pkg.EpisodeLog(n_agents=3, batch=4, gamma=0.9, capacity=8).state_dict()
    with pytest.raises(ValueError, match="gamma = 0.9, this one has 0.8"):
        pkg.EpisodeLog(n_agents=3, batch=4, gamma=0.8, capacity=8).load_state_dict(sd)
    with pytest.raises(ValueError, match="batch = 4, this one has 5"):
        pkg.EpisodeLog(n_agents=3, batch=5, gamma=0.9, capacity=8).load_state_dict(sd)


# ---- the refusals of a resume ----
CONFIG = {"num_steps": 41, "batch": 96, "imposter_model_args": {"layer_dims": [36, 256, 6]}, "crew_model_args": None, "gamma": 0.9,
          "experiment_base_dir": "/somewhere/else", "learning_rate": 0.001}


def _run_dir(tmp_path, config=CONFIG):
    d = tmp_path / "run"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(config, indent=4, default=str))
    return d


def _listing(d):
    return sorted((p.name, p.read_bytes()) for p in d.iterdir())


def test_config_comparison_names_key_and_both_values(pkg, tmp_path):
    tl = pkg.train_loop
    d = _run_dir(tmp_path)
    before = _listing(d)
    tl.check_resume_config("run_experiment", dict(CONFIG, experiment_base_dir="/another/base"), d)  # (the one key that may differ)
    with pytest.raises(ValueError, match=r"run_experiment: .*gamma is 0\.8 in this call and 0\.9 in the run's config\.json"):
        tl.check_resume_config("run_experiment", dict(CONFIG, gamma=0.8), d)
    with pytest.raises(ValueError, match=r"batch is 64 in this call and 96 in the run's config\.json"):
        tl.check_resume_config("run_experiment", dict(CONFIG, batch=64), d)
    with pytest.raises(ValueError, match=r"imposter_model_args is \{'layer_dims': \[36, 128, 6\]\} in this call and \{'layer_dims': \[36, 256, 6\]\}"):
        tl.check_resume_config("run_experiment", dict(CONFIG, imposter_model_args={"layer_dims": [36, 128, 6]}), d)
    with pytest.raises(ValueError, match=r"seed is 3 in this call and '<absent>' in the run's config\.json"):
        tl.check_resume_config("run_sweep", dict(CONFIG, seed=3), d)
    with pytest.raises(ValueError, match=r"learning_rate is '<absent>' in this call and 0\.001"):
        tl.check_resume_config("run_sweep", {k: v for k, v in CONFIG.items() if k != "learning_rate"}, d)
    with pytest.raises(FileNotFoundError, match="no config.json"):
        tl.check_resume_config("run_experiment", CONFIG, tmp_path)
    assert _listing(d) == before  # a refused resume writes nothing


def _snapshot(pkg, **over):
    return dict({"format": pkg.train_loop.RUN_STATE_FORMAT, "abi_version": pkg._lib.ABI_VERSION, "finished": False, "completed_ticks": 16,
                 "payload": torch.arange(5)}, **over)


def test_missing_other_abi_and_finished_snapshots_are_refused_each_with_its_own_message(pkg, tmp_path):
    d = _run_dir(tmp_path)
    with pytest.raises(FileNotFoundError, match=r"there is no run_state\.pt"):
        pkg.read_run_state(d)
    pkg.write_run_state(d, _snapshot(pkg))
    assert torch.equal(pkg.read_run_state(d)["payload"], torch.arange(5))
    pkg.write_run_state(d, _snapshot(pkg, abi_version=pkg._lib.ABI_VERSION + 1))
    with pytest.raises(ValueError, match=rf"written under SUSNET_ABI_VERSION {pkg._lib.ABI_VERSION + 1}, this library is version {pkg._lib.ABI_VERSION}"):
        pkg.read_run_state(d)
    pkg.write_run_state(d, _snapshot(pkg, finished=True, completed_ticks=41))
    with pytest.raises(ValueError, match="the snapshot of a finished run"):
        pkg.read_run_state(d)
    pkg.write_run_state(d, _snapshot(pkg, format=0))
    with pytest.raises(ValueError, match="not a run snapshot of format"):
        pkg.read_run_state(d)
    assert sorted(p.name for p in d.iterdir()) == ["config.json", "run_state.pt"]  # one file, the latest; no temporary left


# ---- the atomic write ----
def test_a_failed_write_leaves_no_partial_file_and_keeps_the_previous_one(pkg, tmp_path, monkeypatch):
    tl = pkg.train_loop
    d = _run_dir(tmp_path)
    real_save = torch.save
    seen = {}

    def failing_save(obj, f, *a, **kw):
        f.write(b"half a snapsh")  # something reaches the disk, under the temporary name
        f.flush()
        seen["names"] = sorted(p.name for p in d.iterdir())
        raise OSError("disk full")

    # no snapshot yet: a failed write leaves none
    monkeypatch.setattr(tl.torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        pkg.write_run_state(d, _snapshot(pkg))
    assert "run_state.pt" not in seen["names"] and len(seen["names"]) == 2  # config.json + the temporary, in the SAME directory
    assert sorted(p.name for p in d.iterdir()) == ["config.json"]
    # a snapshot is there: it survives, byte for byte
    monkeypatch.setattr(tl.torch, "save", real_save)
    path = pkg.write_run_state(d, _snapshot(pkg, completed_ticks=6))
    good = path.read_bytes()
    monkeypatch.setattr(tl.torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        pkg.write_run_state(d, _snapshot(pkg, completed_ticks=11))
    assert "run_state.pt" in seen["names"] and len(seen["names"]) == 3
    assert sorted(p.name for p in d.iterdir()) == ["config.json", "run_state.pt"] and path.read_bytes() == good
    monkeypatch.setattr(tl.torch, "save", real_save)
    assert pkg.read_run_state(d)["completed_ticks"] == 6
    pkg.write_run_state(d, _snapshot(pkg, completed_ticks=11))
    assert pkg.read_run_state(d)["completed_ticks"] == 11
