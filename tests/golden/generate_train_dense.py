#!/usr/bin/env python3
"""Golden vectors of the reference trainer's learning step on a game and on layer stacks the compiled-in layouts do not know (container only).

    python tests/golden/generate_train_dense.py        # rewrites tests/golden/dense/dense_train_*.npz

`run` and `ring_from_populate` are generate_train.py's, unchanged: the UNMODIFIED `DQNTeamTrainer.train_step` with `torch.optim.Adam` on a
reference `ReplayBuffer`.  What differs is the input: base 9x9 1v3 with 5 jobs (F = 78 / 11: no compiled-in layout), hidden stacks of two and
of six layers, and -- random play ends too few episodes in 256 rows -- `dones` set on every 8th ring row BEFORE the reference trains on it
(recorded in `meta`: the input is ours, every output is the reference's).  The files are written as dense/dense_train_<name>.npz: neither
the model_train_* glob of train_fixtures.py nor the suite's glob over the trajectory files in this directory sees them.
tests/test_train_dense_host.py (the package's torch path) and tests/test_gpu_mlp_train.py (susnet_mlp_train_step) are compared with them.
"""
from __future__ import annotations

import json
import os

import numpy as np

import generate_train as gt  # noqa: E402  (installs the import shims)

HERE = gt.HERE
ROWS, DONE_EVERY = 256, 8


def ring_with_dones(spec, seed):
    ring = gt.ring_from_populate(spec, ROWS, seed)
    natural = int(ring["dones"].sum())
    ring["dones"] = ring["dones"].copy()
    ring["dones"].reshape(-1)[::DONE_EVERY] = 1
    return ring, natural


def run_dense(name, spec, seed, components, hidden, batch_sizes):
    ring, natural = ring_with_dones(spec, seed)
    assert int(ring["dones"].sum()) >= 8
    gt.run(name, spec, ring, components, hidden, True, True, 0.9, 1e-2, batch_sizes, seed)
    src, dst = os.path.join(HERE, f"model_train_{name}.npz"), os.path.join(HERE, "dense", f"dense_train_{name}.npz")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    d = np.load(src)
    meta = json.loads(str(d["meta"]))
    meta.update(dones_set_every=DONE_EVERY, done_rows_from_play=natural)
    np.savez_compressed(dst, meta=json.dumps(meta), **{k: d[k] for k in d.files if k != "meta"})
    d.close()
    os.remove(src)
    print(name, "->", os.path.basename(dst), os.path.getsize(dst), "bytes; done rows", meta["done_rows"], "of which from play", natural)
    assert os.path.getsize(dst) < 256 * 1024


def main():
    base9 = {"class": "base", "kwargs": dict(n_imposters=1, n_crew=3, n_jobs=5, shuffle_imposter_index=True, max_time_steps=60)}
    base9["grid"] = gt.make_env(base9).grid.astype(int).tolist()  # the reference's own 9x9 four-room map, recorded for the tests
    sizes = [32] * 12
    sizes[3], sizes[7] = 1, 3
    run_dense("base9_1v3_j5_comps3", base9, 21, ["onehot_pos", "alive_crew", "closest_crew"], (48, 24), sizes)
    run_dense("base9_1v3_j5_coord_deep", base9, 22, ["coord_pos", "alive_crew"], (40, 33, 20, 12, 9, 8), sizes)


if __name__ == "__main__":
    main()
