"""Per-episode info counters on the MI355X: ``susnet_episode_info`` as the stepping kernels emit it where an episode ends
(``susnet_step_io.ep_info`` / ``susnet_feed_io.ep_info``) and as ``susnet_episode_stats`` carries it into the log parallel to the episode
records.  Pinned to the reference by the 13-counter ``metrics`` rows of the step traces under tests/golden/."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden, trace_names

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_fixtures as ef  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
SENTINEL = 0x5A5A5A5A
# the first nine columns of a trace's `metrics` row (SusMetrics order) <- record field
COLUMNS = ("imp_killed_crew", "imp_voted_out", "crew_voted_out", "sabotaged_jobs", "completed_jobs", None, "time_steps", "imposter_won", "crew_won")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("sus-net_amd")


def np_(t):
    return t.detach().cpu().numpy()


def records_of(pkg, words):
    """[..., 4] int32 words -> the nine counters [..., 9] in SusMetrics order (int64)."""
    rec = pkg.episodes.info_records(words)
    L = pkg._lib
    cols = []
    for c in COLUMNS:
        if c is None:
            cols.append(np.zeros(rec.shape, np.int64))
        elif c == "imposter_won":
            cols.append(((rec["outcome"] & L.OUTCOME_IMPOSTER_WON) != 0).astype(np.int64))
        elif c == "crew_won":
            cols.append(((rec["outcome"] & L.OUTCOME_CREW_WON) != 0).astype(np.int64))
        else:
            cols.append(rec[c].astype(np.int64))
    return np.stack(cols, axis=-1)


# ------------------------------------------------------------------------------------------------
# the reference pin: every step trace, TAPE handles, susnet_step with ep_info given
# ------------------------------------------------------------------------------------------------
def env_from_meta(pkg, meta, batch, **kw):
    cls = meta["class"]
    k = dict(meta["kwargs"])
    k.pop("include_walls", None)
    grid = np.array(meta["grid_used"], dtype=bool)
    if cls == "itg":
        return pkg.BatchedImposterTrainingGround(**k, grid=grid, batch=batch, **kw)
    if cls == "tagging":
        return pkg.BatchedFourRoomEnvWithTagging(**k, grid=grid, batch=batch, **kw)
    return pkg.BatchedFourRoomEnv(**k, grid=grid, batch=batch, **kw)


def families():
    fam = {}
    for n in trace_names():
        m = re.match(r"(.*)_s(\d+)$", n)
        fam.setdefault(m.group(1) if m else n, []).append(n)
    return fam


FAMILIES = families()


@pytest.mark.parametrize("kernels", ["compiled", "generic"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_step_emits_the_reference_info_at_every_episode_end(pkg, family, kernels, monkeypatch):
    """Replay of the trace with the recorded actions: at every step that ends an episode the record equals the first nine columns of the
    fixture's `metrics` row; the slot of every other step keeps the sentinel it was filled with."""
    if kernels == "generic":
        monkeypatch.setenv("SUSNET_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("SUSNET_FORCE_GENERIC", raising=False)
    gs = [load_golden(f"{GOLDEN_DIR}/{n}.npz") for n in FAMILIES[family]]
    meta = gs[0]["meta"]
    B = len(gs)
    tagging = meta["class"] == "tagging"
    env = env_from_meta(pkg, meta, B, rng="numpy", reward_dtype=torch.float64, tape_words=1 << 15)
    env._reseed([g["meta"]["seed"] for g in gs])
    env.reset()
    info = torch.zeros(B, 4, dtype=torch.int32, device=env.device)
    env._step_io.ep_info = info.data_ptr()
    sampled = meta["mode"] == "sampled"
    for s in range(len(gs[0]["done"])):
        if s > 0:
            mask = np.array([bool(g["ep_start"][s]) for g in gs])
            if mask.any():
                env.reset(mask=mask)
        if not sampled:
            for g in gs:
                assert B == 1
                if g["inject"][s]:
                    kw = dict(agent_positions=g["pre_pos"][s][None], alive_agents=g["pre_alive"][s][None], t=g["pre_t"][s:s + 1])
                    if env.n_jobs:
                        kw.update(job_positions=g["pre_jobpos"][s][None], completed_jobs=g["pre_jobdone"][s][None])
                    if tagging:
                        kw.update(used_tag_actions=g["pre_used"][s][None], tag_counts=g["pre_counts"][s][None],
                                  tag_reset_timer=g["pre_timer"][s:s + 1])
                    env.set_state(**kw)
        want_a = np.stack([g["actions"][s] for g in gs])
        a = env.sample_actions().clone() if sampled else torch.as_tensor(want_a.astype(np.int64))
        assert np.array_equal(np_(a), want_a)
        info.fill_(SENTINEL)
        _, _, done, trunc, _ = env.step(a)
        words = np_(info)
        got = records_of(pkg, words)
        for b, g in enumerate(gs):
            ended = bool(g["done"][s]) or bool(g["trunc"][s])
            assert (bool(np_(done)[b]) or bool(np_(trunc)[b])) == ended
            if ended:
                want = np.asarray(g["metrics"][s][:9], dtype=np.int64)
                assert got[b].tolist() == want.tolist(), f"{g['name']} step {s}"
            else:
                assert (words[b] == SENTINEL).all(), f"{g['name']} step {s}: a step that ended nothing wrote its slot"


def test_the_traces_hold_the_ends_the_pin_needs():
    """The replays above are parametrised over every trace, none skipped; together the traces end 372 episodes, every counter but
    total_stalemates is non-zero at some end, and kills go beyond what one episode from a reset can reach (injected states)."""
    assert sum(len(v) for v in FAMILIES.values()) == 55
    ends, total, top = 0, np.zeros(9, np.int64), np.zeros(9, np.int64)
    for n in trace_names():
        g = load_golden(f"{GOLDEN_DIR}/{n}.npz")
        ended = np.asarray(g["done"]).astype(bool) | np.asarray(g["trunc"]).astype(bool)
        rows = np.asarray(g["metrics"])[ended][:, :9].astype(np.int64)
        ends += len(rows)
        total += rows.sum(axis=0)
        if len(rows):
            top = np.maximum(top, rows.max(axis=0))
    assert ends == 372
    for i, c in enumerate(COLUMNS):
        assert (total[i] > 0) == (c is not None), c
    assert 15 < top[0] <= 255 and top[1] <= 255 and top[2] <= 255, "the byte-sized fields hold every recorded value"


# ------------------------------------------------------------------------------------------------
# the policy kernels: blocks equal ticks, the env's own books, the parallel log, NULL = today
# ------------------------------------------------------------------------------------------------
def game(pkg, name, batch, seed=5, max_time_steps=30):
    if name == "1v2":
        comps = COMPS3
        env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=seed, auto_reset=True, grid_size=14,
                                     shuffle_imposter_index=True, max_time_steps=max_time_steps, obs=pkg.ObsConfig("flat", comps), check_errors=False)
    else:
        comps = ["onehot_pos"]
        kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
        env = pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device="cuda:0", rng="philox", seed=seed,
                                                auto_reset=True, max_time_steps=max_time_steps, obs=pkg.ObsConfig("flat", comps), check_errors=False)
    net = pkg.policy.pack_mlp(env, pkg.policy.reference_imposter_mlp(env, comps, seed=3), comps)
    assert net is not None
    return env, net


FEED_KEYS = ("actions", "rewards", "done", "truncated", "obs", "term_obs", "roles")


def state_of(pkg, env):
    return {"raw": env.observe(pkg.ObsConfig("raw", dtype=torch.uint8)).clone(), "life": env.lifetime_totals().clone(), "cursor": env.rng_cursor().clone()}


def check_slots(pkg, feed, T):
    """ep_info is written at the ended slots (an episode has at least one step) and nowhere else (the feed is allocated zeroed)."""
    ended = np_(feed["done"][:T] | feed["truncated"][:T])
    words = np_(feed["ep_info"][:T])
    assert (words[~ended] == 0).all()
    assert (pkg.episodes.info_records(words)["time_steps"][ended] >= 1).all()
    return ended


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("name,B", [("1v1", 2088), ("1v2", 2096)])  # (ragged last waves; batch x state size a multiple of 16)
def test_a_block_emits_what_its_ticks_emit(pkg, name, B, eps):
    T = 64
    env, net = game(pkg, name, B, max_time_steps=20)
    twin, net2 = game(pkg, name, B, max_time_steps=20)
    env.reset()
    twin.reset()
    feed, feed2 = env.alloc_feed(T), twin.alloc_feed(T)
    for block in range(2):
        env.policy_rollout_into(feed, T, net, epsilon=eps)
        for t in range(T):
            twin.policy_tick_into(feed2, t, net_imposter=net2, epsilon=eps)
        torch.cuda.synchronize()
        for k in FEED_KEYS + ("ep_info",):
            assert torch.equal(feed[k], feed2[k]), (k, block)
        ended = check_slots(pkg, feed, T)
        assert (ended.sum(axis=0) >= 2).any(), "some environment must end more than once inside one launch"
        feed["ep_info"].zero_()
        feed2["ep_info"].zero_()


@pytest.mark.parametrize("name,B", [("1v1", 2088), ("1v2", 2096)])
def test_info_log_sums_equal_the_lifetime_deltas(pkg, name, B):
    T, blocks = 64, 40  # 2 560 ticks
    env, net = game(pkg, name, B, max_time_steps=30)
    env.reset()
    life0 = np_(env.lifetime_totals()).copy()
    log = pkg.EpisodeLog(env, gamma=0.9, capacity=B * T * blocks)
    feed = env.alloc_feed(T)
    for _ in range(blocks):
        env.policy_rollout_into(feed, T, net, epsilon=0.2)
        log.update(feed, T)
    rec = log.records()
    life = dict(zip(pkg._lib.LIFETIME_NAMES, (np_(env.lifetime_totals()) - life0).tolist()))
    assert rec["dropped"] == 0 and rec["count"] == life["episodes"] > B
    assert int(rec["imposter_won"].sum()) == life["imposter_won"] and int(rec["crew_won"].sum()) == life["crew_won"]
    assert int(((rec["ended_by"] & pkg._lib.EPISODE_TRUNCATED) != 0).sum()) == life["truncated"]
    for k in ("imp_killed_crew", "imp_voted_out", "crew_voted_out", "sabotaged_jobs", "completed_jobs"):
        assert int(rec[k].sum()) == life[k], k
    assert int(rec["total_time_steps"].sum()) == life["episode_steps"]
    assert life["imposter_won"] > 0 and life["truncated"] > 0 and life["imp_killed_crew"] > 0
    if name == "1v2":
        assert life["completed_jobs"] > 0 and life["crew_won"] + life["imposter_won"] + life["truncated"] >= life["episodes"]
    assert np.array_equal(rec["total_time_steps"], rec["length"])  # (the log started with the run)
    # evaluate(): the same loop behind one call; its rates are the lifetime deltas of its own run
    model = pkg.policy.reference_imposter_mlp(env, env.obs_config.components, seed=3)
    before = np_(env.lifetime_totals()).copy()
    out = pkg.evaluate(env, model, None, env.obs_config.components, 640, epsilon=0.0)
    d = dict(zip(pkg._lib.LIFETIME_NAMES, (np_(env.lifetime_totals()) - before).tolist()))
    assert out["episodes"] == d["episodes"] > 0 and out["dropped"] == 0 and out["ticks"] == 640
    assert out["imposter_win_rate"] == d["imposter_won"] / d["episodes"] and out["crew_win_rate"] == d["crew_won"] / d["episodes"]
    assert out["truncation_rate"] == d["truncated"] / d["episodes"] and out["mean_length"] == d["episode_steps"] / d["episodes"]
    assert out["mean_imp_killed_crew"] == d["imp_killed_crew"] / d["episodes"] and out["mean_completed_jobs"] == d["completed_jobs"] / d["episodes"]


def host_feed(feed, T):
    return {k: np_(feed[k][:T]) for k in ("rewards", "done", "truncated", "roles", "ep_info")}


def assert_logs_equal(got, want):
    ef.assert_records_equal(got, want, n=want["count"])
    assert got["dropped"] == want["dropped"]
    for k in ("imp_killed_crew", "imp_voted_out", "crew_voted_out", "sabotaged_jobs", "completed_jobs", "total_time_steps", "imposter_won", "crew_won"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("capacity", [1 << 16, 777])
def test_info_log_is_parallel_to_the_episode_log(pkg, capacity):
    B, T = 2096, 48
    env, net = game(pkg, "1v2", B, max_time_steps=12)
    env.reset()
    dev = pkg.EpisodeLog(env, gamma=0.9, capacity=capacity)
    host = pkg.EpisodeLog(gamma=0.9, capacity=capacity, n_agents=env.n_agents, batch=B)
    feed = env.alloc_feed(T)
    for n in (T, 17):  # a log carried over two update calls
        feed["ep_info"].zero_()
        env.policy_rollout_into(feed, n, net, epsilon=0.1)
        dev.update(feed, n)
        torch.cuda.synchronize()
        host.update(host_feed(feed, n), n)
    got, want = dev.records(), host.records()
    assert want["count"] == min(capacity, want["count"] + want["dropped"]) and (want["dropped"] > 0) == (capacity == 777)
    assert want["count"] > 500
    assert_logs_equal(got, want)


@pytest.mark.parametrize("name,B", [("1v1", 2088), ("1v2", 2096)])
def test_null_pointers_are_today(pkg, name, B):
    """Without ep_info / info the states, feeds and episode records equal those of a twin run with the pointers given."""
    T = 40
    env, net = game(pkg, name, B, max_time_steps=15)
    twin, net2 = game(pkg, name, B, max_time_steps=15)
    env.reset()
    twin.reset()
    feed, feed2 = env.alloc_feed(T), twin.alloc_feed(T)
    del feed2["ep_info"]
    log, log2 = pkg.EpisodeLog(env, gamma=0.9, capacity=1 << 16), pkg.EpisodeLog(twin, gamma=0.9, capacity=1 << 16)
    for step in range(2):
        env.policy_rollout_into(feed, T, net, epsilon=0.1)
        twin.policy_rollout_into(feed2, T, net2, epsilon=0.1)
        log.update(feed, T)
        log2.update(feed2, T)
        env.policy_tick_into(feed, 0, net_imposter=net, epsilon=0.1)
        twin.policy_tick_into(feed2, 0, net_imposter=net2, epsilon=0.1)
        torch.cuda.synchronize()
        for k in FEED_KEYS:
            assert torch.equal(feed[k], feed2[k]), (k, step)
        log.update(feed, 1)
        log2.update(feed2, 1)
        feed["ep_info"].zero_()
    # ... and the plain step API (susnet_step) with and without the pointer
    info = torch.zeros(B, 4, dtype=torch.int32, device=env.device)
    env._step_io.ep_info = info.data_ptr()
    ends = 0
    for _ in range(30):
        a = env.sample_actions().clone()
        assert torch.equal(a, twin.sample_actions())
        _, r1, d1, t1, _ = env.step(a)
        _, r2, d2, t2, _ = twin.step(a)
        assert torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(t1, t2)
        ends += int((d1 | t1).sum())
    assert ends > 0 and int((info != 0).any(dim=1).sum()) > 0
    a, b = state_of(pkg, env), state_of(pkg, twin)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    got, want = log.records(), log2.records()
    assert got["count"] == want["count"] > B and "imposter_won" in got and "imposter_won" not in want
    ef.assert_records_equal(got, want)


def test_run_experiment_writes_one_info_entry_per_episode(pkg, tmp_path):
    import json

    env, _ = game(pkg, "1v2", 256, max_time_steps=30)
    comps = COMPS3
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    crew = pkg.policy.reference_crew_mlp(env, comps, seed=4)
    life0 = np_(env.lifetime_totals()).copy()
    metrics = pkg.run_experiment(env, num_steps=64, imposter_model=imp, crew_model=crew, components=comps, replay_buffer_size=50_000,
                                 replay_prepopulate_steps=0, batch_size=32, gamma=0.9, scheduler_time_steps=40, experiment_base_dir=tmp_path,
                                 learning_rate=1e-3, train_step_interval=5, target_update_interval=16)
    life = dict(zip(pkg._lib.LIFETIME_NAMES, (np_(env.lifetime_totals()) - life0).tolist()))
    (run_dir,) = list(tmp_path.iterdir())
    saved = json.loads((run_dir / "metrics.json").read_text())
    n_ep = life["episodes"]
    assert n_ep >= 2 * env.batch  # (max_time_steps = 30: every env finishes two episodes in 64 ticks)
    for name, total in (("imp_killed_crew", life["imp_killed_crew"]), ("imp_voted_out", 0), ("crew_voted_out", 0), ("sabotaged_jobs", life["sabotaged_jobs"]),
                        ("completed_jobs", life["completed_jobs"]), ("total_stalemates", 0), ("total_time_steps", life["episode_steps"]),
                        ("imposter_won", life["imposter_won"]), ("crew_won", life["crew_won"])):
        assert len(saved[name]) == n_ep == len(metrics.metrics[pkg.SusMetrics(name)]) and sum(saved[name]) == total, name
    assert len(saved["avg_imposter_returns"]) == n_ep
    curve = np.convolve(np.asarray(saved["imposter_won"], dtype=np.float64), np.ones(50) / 50, mode="valid")
    assert len(curve) == n_ep - 49 and 0 <= curve.min() <= curve.max() <= 1
    # ... and the checkpoints it wrote, as a table over training progress
    table = pkg.evaluate_checkpoints(run_dir, env, comps, 64)
    assert list(table) == ["0", "25", "50", "75", "100%"] and all(v["episodes"] >= env.batch for v in table.values())
