"""Shared by the episode-bookkeeping tests: the reference train() recordings of tests/golden/episodes/episodes_*.npz as feed blocks."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episodes")
FIELDS = ("imposter_return", "crew_return", "length", "tick", "env", "ended_by")


def names():
    return sorted(os.path.basename(p)[len("episodes_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "episodes_*.npz")))


def load(name):
    """-> dict: ``feed`` (rewards [T, 1, A] float32, done / truncated [T, 1] bool, roles [T, 1] int16 bitmask), ``gamma``, ``n_agents`` and the
    reference's lists ``imposter_return``, ``crew_return``, ``length`` plus the derived ``tick`` and ``ended_by`` of every finished episode."""
    d = np.load(os.path.join(GOLDEN, f"episodes_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    reward, done, trunc = d["reward"], d["done"].astype(bool), d["trunc"].astype(bool)
    roles = np.zeros(len(reward), dtype=np.int64)
    for col in d["imposters"].T:
        roles |= 1 << col.astype(np.int64)
    ends = np.flatnonzero(done | trunc)
    return {
        "name": name, "meta": meta, "gamma": float(d["gamma"]), "n_agents": reward.shape[1],
        "feed": {"rewards": reward[:, None, :].copy(), "done": done[:, None].copy(), "truncated": trunc[:, None].copy(),
                 "roles": roles.astype(np.int16)[:, None].copy()},
        "imposter_return": d["avg_imposter_returns"], "crew_return": d["avg_crew_returns"], "length": d["total_time_steps"].astype(np.int32),
        "tick": ends.astype(np.int64), "env": np.zeros(len(ends), dtype=np.int32),
        "ended_by": (done[ends].astype(np.int32) * 1 + trunc[ends].astype(np.int32) * 2),
    }


def slice_feed(feed, t0, t1):
    return {k: v[t0:t1] for k, v in feed.items()}


def uneven_blocks(total, sizes=(1, 5, 5, 3, 64, 7, 130, 2)):
    """(t0, t1) pairs covering 0 .. total with the block sizes cycling through ``sizes``."""
    out, t, i = [], 0, 0
    while t < total:
        n = min(sizes[i % len(sizes)], total - t)
        out.append((t, t + n))
        t, i = t + n, i + 1
    return out


def assert_records_equal(got, want, n=None):
    """Every field exactly; the float64 returns bit for bit (NaN-free by construction)."""
    n = len(want["tick"]) if n is None else n
    assert got["count"] == n, (got["count"], n)
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])[:n]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.int64), b.astype(np.float64).view(np.int64)), (k, np.flatnonzero(a != b)[:5])
        else:
            assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:5])


def merged_streams(fixtures, batch, total_ticks):
    """Env b replays fixture stream ``b mod K`` rotated by ``b`` ticks.  -> feed arrays ``[total_ticks, batch, A]`` (all fixtures must have the
    same agent count) and one (feed of env b) list for the per-env expectation."""
    K = len(fixtures)
    A = fixtures[0]["n_agents"]
    assert all(f["n_agents"] == A for f in fixtures)
    feed = {"rewards": np.zeros((total_ticks, batch, A), np.float32), "done": np.zeros((total_ticks, batch), bool),
            "truncated": np.zeros((total_ticks, batch), bool), "roles": np.zeros((total_ticks, batch), np.int16)}
    for b in range(batch):
        src = fixtures[b % K]["feed"]
        T = src["rewards"].shape[0]
        idx = (np.arange(total_ticks) + b) % T
        for k in feed:
            feed[k][:, b] = src[k][idx, 0]
    return feed
