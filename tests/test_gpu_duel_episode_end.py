"""The episode-end path of the 1v1 fused rollout (k_rollout_duel) where it is busiest: episodes of 2 and 7 steps, so that some lane of a
wave finishes on almost every tick, lanes finish twice before the wave draws new spawn cells, and launches of 1, 11, 12, 13, 24, 25 and
37 ticks in sequence on one handle (the unrolled group is 12 ticks: a launch that is exactly one group, one that ends one tick behind a
group, starts that are not group-aligned, and always a last tick whose info counters must stay readable).  Against the CPU oracle, tick by
tick, in every output mode of the kernel."""
import numpy as np
import pytest

from test_gpu_parity import CONFIGS, compare_full_state, make_pair, np_, pkg  # noqa: F401  (pkg: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAUNCHES = (1, 11, 12, 13, 24, 25, 37)
GAMES = ("itg_1v1_nowalls", "itg_1v1_walls")
SEED = 2  # (chosen on the oracle alone: at B >= 96 every game and episode length has a tick where a landed kill meets the truncation)
# mode -> (packed, replay_feed)
MODES = {"compact": ("compact", False), "record20": (True, False), "tensors": (False, False), "tensors-feed": (False, True),
         "compact-feed": ("compact", True), "record20-feed": (True, True)}
K_KILLS, K_STEPS = 0, 6  # oracle.METRIC_NAMES: imp_killed_crew, total_time_steps
L_EPISODES, L_CREW_WON, L_IMP_WON, L_TRUNC, L_KILLS, L_EP_STEPS, L_ENV_STEPS = 0, 1, 2, 3, 4, 9, 10  # _lib.LIFETIME_NAMES


class _Snapshot:
    """What compare_full_state reads of an OracleBatch, kept from the tick it was taken at."""

    def __init__(self, export):
        self._e = {k: np.array(v, copy=True) for k, v in export.items()}

    def export(self):
        return self._e


def _pair(pkg, oracle_mod, name, B, max_t, **envkw):
    short = f"{name}@{max_t}"
    CONFIGS[short] = dict(CONFIGS[name], kw=dict(CONFIGS[name]["kw"], max_time_steps=max_t))
    try:
        return make_pair(pkg, oracle_mod, short, B, SEED, auto_reset=True, check_errors=False, **envkw)
    finally:
        del CONFIGS[short]


_REFERENCE = {}


def reference(pkg, oracle_mod, name, B, max_t):
    """The oracle's run of the launch sequence, computed once per (game, batch, episode length) and shared by every mode: per launch the
    per-tick outputs, the terminal rows, the state / info counters / lifetime sums after it."""
    key = (name, B, max_t)
    if key in _REFERENCE:
        return _REFERENCE[key]
    env, ob = _pair(pkg, oracle_mod, name, B, max_t)
    del env
    ob.reset()
    life = np.zeros(12, np.int64)
    launches, both, ended_total = [], 0, np.zeros(B, np.int64)
    for n in LAUNCHES:
        ticks = []
        for s in range(n):
            oa = ob.sample_actions()
            orew, odone, otrunc, rc = ob.step(oa)
            assert rc == 0
            ended = (odone | otrunc).astype(bool)
            m = ob.export()["metrics"].copy()  # before the reset: the finished episodes' counters
            term = ob.obs_raw_u8().copy()
            both += int((odone.astype(bool) & otrunc.astype(bool)).sum())
            life[L_EPISODES] += int(ended.sum())
            life[L_IMP_WON] += int(odone.astype(bool).sum())
            life[L_TRUNC] += int(otrunc.astype(bool).sum())
            life[L_KILLS] += int(m[ended, K_KILLS].sum())
            life[L_EP_STEPS] += int(m[ended, K_STEPS].sum())
            life[L_ENV_STEPS] += B
            ended_total += ended
            ob.reset(mask=ended)
            ticks.append(dict(actions=oa.copy(), rewards=orew.copy(), done=odone.astype(bool), trunc=otrunc.astype(bool), ended=ended, term=term,
                              obs=ob.obs_raw_u8().copy(), info=m))
        launches.append(dict(n=n, ticks=ticks, state=_Snapshot(ob.export()), life=life.copy()))
    ref = dict(launches=launches, both=both, min_ended=int(ended_total.min()))
    _REFERENCE[key] = ref
    return ref


def _launch(pkg, env, n, mode, record=None):
    packed, feed = MODES[mode]
    obs_cfg = pkg.ObsConfig("raw", dtype=torch.uint8)
    bufs = env.alloc_rollout(n, obs=obs_cfg, packed=packed, replay_feed=feed)
    if record is not None:  # the caller's own record buffer (guard rows around it)
        for k in ("actions", "rewards", "done", "truncated", "obs"):
            bufs.pop(k, None)
        bufs["record"] = record
    env.rollout_into(n, bufs)
    torch.cuda.synchronize()
    if packed and "actions" not in bufs:
        bufs.update(env.record_fields(bufs["record"], packed))
    return bufs


def _check_launch(env, bufs, lr, mode, tag, ticks_so_far):
    feed = MODES[mode][1]
    acts, rews, dones, truncs, obs = (np_(bufs[k]) for k in ("actions", "rewards", "done", "truncated", "obs"))
    term = np_(bufs["term_obs"]) if feed else None
    for s, t in enumerate(lr["ticks"]):
        np.testing.assert_array_equal(acts[s], t["actions"], err_msg=f"{tag} actions tick {s}")
        assert np.array_equal(rews[s].astype(np.float64).view(np.uint64), t["rewards"].view(np.uint64)), f"{tag} rewards tick {s}"
        np.testing.assert_array_equal(dones[s].astype(bool), t["done"], err_msg=f"{tag} done tick {s}")
        np.testing.assert_array_equal(truncs[s].astype(bool), t["trunc"], err_msg=f"{tag} truncated tick {s}")
        np.testing.assert_array_equal(obs[s], t["obs"], err_msg=f"{tag} raw obs tick {s}")
        if feed:  # the terminal state where the oracle's episode ended, untouched (zero) rows elsewhere
            np.testing.assert_array_equal(term[s][t["ended"]], t["term"][t["ended"]], err_msg=f"{tag} terminal rows tick {s}")
            assert not term[s][~t["ended"]].any(), f"{tag} terminal rows written where no episode ended, tick {s}"
    if feed and "roles" in bufs:
        assert (np_(bufs["roles"])[:lr["n"]] == 1).all(), f"{tag} roles"
    env._export(full=True)
    compare_full_state(env, lr["state"], tag)
    # the info counters of the launch's last tick stay readable, also for environments whose episode ended on it
    np.testing.assert_array_equal(np_(env._metrics), lr["ticks"][-1]["info"], err_msg=f"{tag} info counters")
    life = np_(env.lifetime_totals()).astype(np.int64)
    np.testing.assert_array_equal(life[:11], lr["life"][:11], err_msg=f"{tag} lifetime totals")
    assert int(env.tick) == ticks_so_far, f"{tag} tick count"


def _assert_reference_is_busy(ref, B, max_t):
    """The cases this file exists for did occur (from the oracle's outputs alone)."""
    # truncation alone ends an episode after max_t steps, so over the 123 ticks every environment finished at least 123 // max_t times:
    # with 2-step episodes six times per 12-tick group, far more often than a wave draws new spawn cells
    assert ref["min_ended"] >= sum(LAUNCHES) // max_t
    if B >= 96:
        assert ref["both"] > 0, "no tick on which a landed kill and the truncation coincide: pick another seed"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("max_t", [2, 7])
@pytest.mark.parametrize("B", [1, 96, 200])
@pytest.mark.parametrize("name", GAMES)
def test_launch_sequence_matches_oracle(pkg, oracle_mod, name, B, max_t, mode):
    ref = reference(pkg, oracle_mod, name, B, max_t)
    _assert_reference_is_busy(ref, B, max_t)
    env, _ = _pair(pkg, oracle_mod, name, B, max_t)
    env.reset()
    done_ticks = 0
    for lr in ref["launches"]:
        bufs = _launch(pkg, env, lr["n"], mode)
        done_ticks += lr["n"]
        _check_launch(env, bufs, lr, mode, f"{name} B={B} max_t={max_t} {mode} launch of {lr['n']}", done_ticks)


@pytest.mark.parametrize("mode", ["compact-feed", "record20-feed", "tensors-feed"])
@pytest.mark.parametrize("max_t", [2, 7])
@pytest.mark.parametrize("name", GAMES)
def test_forced_chunking_equals_the_unchunked_run(pkg, oracle_mod, name, max_t, mode, monkeypatch):
    """Five ticks per launch (SUSNET_TRAJ_MAX_BYTES): every request of the sequence but the first runs as several launches, each with a last
    tick of its own -- record for record (and terminal row for terminal row) what the unchunked handle wrote, and the oracle's state."""
    B = 96
    packed, _ = MODES[mode]
    ref = reference(pkg, oracle_mod, name, B, max_t)
    whole, _ = _pair(pkg, oracle_mod, name, B, max_t)
    tick_bytes = B * whole.record_layout(packed).record_bytes if packed else 8 * B
    monkeypatch.setenv("SUSNET_TRAJ_MAX_BYTES", str(5 * tick_bytes + tick_bytes // 2))
    cut, _ = _pair(pkg, oracle_mod, name, B, max_t)
    monkeypatch.delenv("SUSNET_TRAJ_MAX_BYTES")
    whole.reset()
    cut.reset()
    done_ticks = 0
    for lr in ref["launches"]:
        n = lr["n"]
        bw, bc = _launch(pkg, whole, n, mode), _launch(pkg, cut, n, mode)
        done_ticks += n
        keys = ("record", "term_obs") if packed else ("actions", "rewards", "done", "truncated", "obs", "term_obs", "roles")
        for k in keys:
            assert torch.equal(bw[k], bc[k]), f"{name} max_t={max_t} {mode} launch of {n}: {k} differs under chunking"
        _check_launch(cut, bc, lr, mode, f"{name} max_t={max_t} {mode} chunked launch of {n}", done_ticks)


@pytest.mark.parametrize("packed", ["compact", True], ids=["compact", "record20"])
@pytest.mark.parametrize("epw", [64, 32, 16])
@pytest.mark.parametrize("name", GAMES)
def test_wave_widths_write_nothing_outside_the_records(pkg, oracle_mod, name, epw, packed, monkeypatch):
    """B = 96 at every wave width (a ragged last wave at 64, lanes without an environment in every wave at 32 and 16): the records of the
    launch sequence against the oracle, and guard rows in front of and behind the launch's records keep their sentinel."""
    B, max_t = 96, 2
    mode = "compact" if packed == "compact" else "record20"
    ref = reference(pkg, oracle_mod, name, B, max_t)
    monkeypatch.setenv("SUSNET_EPW", str(epw))
    env, _ = _pair(pkg, oracle_mod, name, B, max_t)
    monkeypatch.delenv("SUSNET_EPW")
    assert env.native_layout().envs_per_wave == epw
    R = env.record_layout(packed).record_bytes
    env.reset()
    done_ticks = 0
    for lr in ref["launches"]:
        n = lr["n"]
        big = torch.full((n + 2, B, R), 0xA5, dtype=torch.uint8, device=env.device)
        bufs = _launch(pkg, env, n, mode, record=big[1:n + 1])
        done_ticks += n
        guard = np_(big)
        assert (guard[0] == 0xA5).all() and (guard[n + 1] == 0xA5).all(), f"{name} epw={epw} launch of {n}: a store left the launch's records"
        _check_launch(env, bufs, lr, mode, f"{name} epw={epw} {mode} launch of {n}", done_ticks)
