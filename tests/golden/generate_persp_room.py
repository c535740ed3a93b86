#!/usr/bin/env python3
"""Golden room-masked Perspective views from the UNMODIFIED reference (container only).

    python tests/golden/generate_persp_room.py       # rewrites tests/golden/persp_room/*.npz

The reference's ``PartiallyObservableFeaturizer`` (src/features/component.py:162-197) has no caller that can construct it as
written: it reads ``agent_state.agent_position``, which nothing provides, and calls ``get_blank_features`` on a composite, which
has no such method.  Here both are PROVIDED, from outside, and its own ``extract_features`` (lines 173-193, with ``ROOM_MASKS``
of lines 8-17) runs unchanged: the composite's one component hands back agent i's view as the reference's
``PerspectiveFeaturizer`` (src/features/model_ready.py:82-216) made it, the agent state carries agent i's position of that
state row, and the blank features are numpy zeros of the grid's shape.

Rows: about 64 states of episodes played with random actions on the reference env, plus directed rows edited into copies of
them, so that the cases ``check_cases`` lists are all there (asserted here, and again by the host test).  Only data is stored,
as uint8: the raw rows, the expected views with and without the mask channel, the non-spatial rows.

Games: base 1v2 with 4 jobs, tagging 1v4 with 5 jobs (two per-agent non-spatial blocks: alive flags and tag counts).  The tagging
env instance gets its ``state_fields`` map put in the order of its own state tuple (see ``main``): without that the reference's
featurizers raise on that env.
"""
from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()
import torch  # noqa: E402

from generate_golden import make_env  # noqa: E402
from src.features import component as comp  # noqa: E402
from src.features.model_ready import PerspectiveFeaturizer  # noqa: E402

OUT_DIR = os.path.join(HERE, "persp_room")
N = 9

GAMES = {
    "base_1v2_j4": (dict(**{"class": "base"}, kwargs=dict(n_imposters=1, n_crew=2, n_jobs=4)), 11),
    "tagging_1v4_j5": (dict(**{"class": "tagging"}, kwargs=dict(n_imposters=1, n_crew=4, n_jobs=5)), 12),
}


class _View(comp.BaseSpatialFeaturizer):
    """The composite's one component: agent i's Perspective view, as the reference featurizer produced it."""

    def __init__(self, env, channels):
        super().__init__(env)
        self.channels = channels

    def extract_features(self, agent_state):
        return agent_state.view

    @property
    def shape(self):
        return torch.tensor([self.channels, N, N], dtype=torch.int)


class _Constructible(comp.PartiallyObservableFeaturizer):
    """What the reference class lacks to run; ``extract_features`` is inherited untouched."""

    def get_blank_features(self, num_channels):
        return np.zeros((num_channels, N, N))


def played_rows(env, seed, n_rows, stride):
    """Every ``stride``-th state of random play (populate()-shaped: reset on done | truncated), ``n_rows`` of them."""
    np.random.seed(seed)
    state, _ = env.reset()
    rows, t = [], 0
    while len(rows) < n_rows:
        if t % stride == 0:
            rows.append(np.asarray(env.flatten_state(state), dtype=np.int64))
        state, _, done, trunc, _ = env.step(env.sample_actions())
        if done or trunc:
            state, _ = env.reset()
        t += 1
    return np.stack(rows)


def directed_rows(base, A, J):
    """Rows edited into copies of played ones: observer 0 placed in each room and on / next to the wall row and column; agents
    and jobs put inside and outside its room, alive and dead, done and not done."""
    out = []

    def edit(src, pos=None, alive=None, jobs=None, done=None):
        r = base[src % len(base)].copy()
        for a, (x, y) in (pos or {}).items():
            r[2 * a], r[2 * a + 1] = x, y
        for a, v in (alive or {}).items():
            r[2 * A + a] = v
        for j, (x, y) in (jobs or {}).items():
            r[3 * A + 2 * j], r[3 * A + 2 * j + 1] = x, y
        for j, v in (done or {}).items():
            r[3 * A + 2 * J + j] = v
        out.append(r)

    everyone = {a: 1 for a in range(A)}
    # observer 0 in each room; agent 1 alive in its room, agent 2 alive outside; one job in, one out, done and not done
    for k, (x, y) in enumerate([(1, 2), (2, 7), (7, 6), (6, 1)]):
        inside, outside = (x, y ^ 1), (8 - x, 8 - y)
        edit(k, pos={0: (x, y), 1: inside, 2: outside}, alive=everyone, jobs={0: inside, 1: outside, 2: (x ^ 1, y), 3: (8 - x, y)},
             done={0: k & 1, 1: k & 1, 2: 1 - (k & 1), 3: 1 - (k & 1)})
    # on the wall row (x = 4), on the wall column (y = 4), right behind them (x = 5 / y = 5), and the crossing itself
    for k, (x, y) in enumerate([(4, 1), (4, 7), (1, 4), (7, 4), (5, 2), (2, 5), (5, 5), (4, 4), (5, 4), (4, 5)]):
        edit(4 + k, pos={0: (x, y), 1: (4, 4), 2: (5, 5)}, alive=everyone, jobs={0: (4, 0), 1: (5, 0), 2: (0, 4), 3: (0, 5)},
             done={0: 0, 1: 1, 2: 1, 3: 0})
    # a dead observer (it keeps its position: its own channel is blank, its mask is its room's), a dead agent inside its room
    edit(20, pos={0: (3, 3), 1: (2, 2), 2: (6, 6)}, alive={0: 1, 1: 0, 2: 1})
    edit(21, pos={0: (6, 2), 1: (7, 1), 2: (1, 1)}, alive={0: 1, 1: 0, 2: 0})
    edit(22, pos={0: (2, 6), 1: (1, 7), 2: (7, 7)}, alive={0: 0, 1: 1, 2: 1})  # (agent 0 dead: as an observer, in its room)
    edit(23, pos={0: (8, 8), 1: (8, 8), 2: (0, 0)}, alive={0: 1, 1: 1, 2: 1})  # two agents on one cell, a corner
    return np.stack(out)


def room_of(x, y):
    return (x <= 4) + 2 * (y <= 4)


def check_cases(rows, A, J):
    """The cases the fixture must contain (the issue's list); the host test repeats these assertions on the stored rows."""
    pos, alive = rows[:, :2 * A].reshape(-1, A, 2), rows[:, 2 * A:3 * A] != 0
    jobs, done = rows[:, 3 * A:3 * A + 2 * J].reshape(-1, J, 2), rows[:, 3 * A + 2 * J:3 * A + 3 * J] != 0
    rooms, jroom = room_of(pos[..., 0], pos[..., 1]), room_of(jobs[..., 0], jobs[..., 1])
    assert set(np.unique(rooms)) == {0, 1, 2, 3}, "an observer in each of the four rooms"
    for axis, v in ((0, 4), (1, 4), (0, 5), (1, 5)):
        assert (pos[..., axis] == v).any(), f"an observer at coordinate {axis} = {v}"
    same = rooms[:, :, None] == rooms[:, None, :]  # [R, observer, other]
    other = ~np.eye(A, dtype=bool)[None]
    assert (same & other & alive[:, None, :]).any() and (~same & alive[:, None, :]).any(), "a living agent inside / outside the observer's room"
    assert (~alive).any(), "a dead observer"
    assert (same & other & ~alive[:, None, :]).any(), "a dead agent inside the observer's room"
    jsame = rooms[:, :, None] == jroom[:, None, :]  # [R, observer, job]
    for inside in (True, False):
        for d in (True, False):
            assert ((jsame == inside) & (done[:, None, :] == d)).any(), f"a job inside={inside} done={d}"


def expected(env, rows):
    """The reference's views of every row: PerspectiveFeaturizer, then component.py:173-193 on each agent's view."""
    A = env.n_agents
    pf = PerspectiveFeaturizer(env)
    pf.fit(torch.tensor(rows.astype(np.float64)).unsqueeze(1))  # [R, T = 1, S]
    views = pf.generate_featurized_states()
    po = {flag: _Constructible([_View(env, A + 2)], add_obs_mask_feature=flag) for flag in (True, False)}
    out = {True: [], False: []}
    for i, (spatial, _) in enumerate(views):
        for flag in (True, False):
            per_row = []
            for r in range(rows.shape[0]):
                state = SimpleNamespace(agent_position=(int(rows[r, 2 * i]), int(rows[r, 2 * i + 1])), view=spatial[r, 0].detach())
                per_row.append(np.asarray(po[flag].extract_features(state)))
            out[flag].append(np.stack(per_row))
    non_spatial = np.stack([v[1][:, 0].detach().numpy() for v in views], axis=1)  # [R, A, F2]
    return np.stack(out[True], axis=1), np.stack(out[False], axis=1), non_spatial


def as_u8(x):
    y = np.asarray(x).astype(np.uint8)
    assert np.array_equal(y, np.asarray(x)), "not uint8-valued"
    return y


def main():
    assert all(m.shape == (N, N) for m in comp.ROOM_MASKS) and np.array_equal(sum(comp.ROOM_MASKS), np.ones((N, N)))
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, (spec, seed) in GAMES.items():
        env = make_env(spec)
        if spec["class"] == "tagging":
            # FourRoomEnvWithTagging's `state_fields` (tagging.py:15-25) order the fields differently from the tuple its own observation
            # space unflattens (42-60), so the reference's spatial featurizers raise on it as it stands (component.py:120-124 reads the
            # alive flags as job positions).  An instance override, like make_env's grid: the map put in the tuple's order -- every
            # field's enum value IS its place in the tuple -- and the reference classes then run unchanged.
            env.state_fields = {field: field.value for field in env.state_fields}
        A, J = env.n_agents, env.n_jobs
        base = played_rows(env, seed, 64, stride=7)
        rows = np.concatenate([base, directed_rows(base, A, J)])
        check_cases(rows, A, J)
        with_mask, without, non_spatial = expected(env, rows)
        assert with_mask.shape == (len(rows), A, A + 3, N, N) and without.shape == (len(rows), A, A + 2, N, N)
        meta = dict(spec, seed=seed, n_agents=int(A), n_jobs=int(J), n_imposters=int(env.n_imposters), grid_n=N, played=len(base))
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), raw=as_u8(rows), spatial_mask=as_u8(with_mask), spatial=as_u8(without),
                            non_spatial=as_u8(non_spatial))
        print(name, "rows =", len(rows), "size =", os.path.getsize(path))


if __name__ == "__main__":
    main()
