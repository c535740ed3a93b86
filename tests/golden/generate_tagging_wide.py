#!/usr/bin/env python3
"""Fixtures of FourRoomEnvWithTagging with 9 .. 12 agents -- three words of agent bytes in the byte-parallel kernels -- from the
UNMODIFIED reference env (container only).

    python tests/golden/generate_tagging_wide.py        # rewrites tests/golden/tagging_wide/*.npz

They live in a directory of their own: tests/golden/ itself holds a counted set of trace fixtures, and every crc_*.npz there runs
through the epw / layout matrix of the existing parametrised tests.  Data only is committed.

  directed_tagging12_votes   2v10, votes every second step, a shuffled action order, states injected (format: generate_golden.py):
                             a count of 11 on an agent of the third word, a 6/6 tie across words 0 and 2, tags before and after a kill
                             on the tagged cell, an imposter voted out by indices 5 .. 11, dead taggers and a dead target
  crc_tagging_*              64 seeds x 96 steps of random play as CRC32 streams (format: generate_checksums.py)
"""
from __future__ import annotations

import json
import os
import zlib

import numpy as np

from generate_golden import METRIC_ORDER, Recorder, run_given  # noqa: F401  (installs the reference shims)
from generate_checksums import N_SEEDS, N_STEPS, run

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tagging_wide")
A, IMPOSTERS = 12, (0, 1)  # shuffle_imposter_index = False: the imposters are agents [0, n_imposters) (base.py:278)
STAY, KILL = 0, 6          # role-relative (base.py:82-99)


def tag(agent, target):
    """The role-relative index of `agent` tagging `target` (tagging.py:68-75: the other agents ascending, behind the role's list)."""
    others = [j for j in range(A) if j != agent]
    return (7 if agent in IMPOSTERS else 6) + others.index(target)


def directed_script():
    spread = [[i % 9, 2 * (i // 9) + (i % 2)] for i in range(A)]  # twelve distinct cells
    fresh = dict(timer=0, counts=[0] * A, used=[0] * A)
    stay = dict(inject=None, actions=[STAY] * A)
    script = []
    # 1. eleven tags on agent 11 (word 2), one on agent 10: the count reaches 11, a crew member of the third word is ejected
    script += [dict(inject=dict(pos=spread, alive=[1] * A, **fresh), actions=[tag(i, 11) for i in range(11)] + [tag(11, 10)]), stay]
    # 2. a 6 / 6 tie at quorum between agents 3 (word 0) and 9 (word 2): the lower index leaves
    script += [dict(inject=dict(pos=spread, alive=[1] * A, **fresh), actions=[tag(i, 9) for i in range(6)] + [tag(i, 3) for i in range(6, 12)]), stay]
    # 3. imposter 0 shares its cell with crew members 4 and 9 and KILLs; everybody else tags one of the two: a tag cast before the
    #    killer's turn counts (and dies with its target), one cast after it on the victim fails and leaves the tagger's vote unused
    pile = [list(p) for p in spread]
    pile[0] = pile[4] = pile[9] = [4, 4]
    script += [dict(inject=dict(pos=pile, alive=[1] * A, **fresh), actions=[KILL] + [tag(i, 9 if i % 2 == 0 else 4) for i in range(1, A)]), stay]
    # 4. agents 5 .. 11 tag imposter 1: voted out with 7 >= quorum 6; the vote reward keeps its sign as coded (tagging.py:196)
    script += [dict(inject=dict(pos=spread, alive=[1] * A, **fresh), actions=[STAY] * 5 + [tag(i, 1) for i in range(5, 12)]), stay]
    # 5. agents 2, 7 and 10 are dead: the dead tag (tagging.py:103-110 never checks the actor), agent 3 tags dead agent 7 (fails)
    dead = [0 if i in (2, 7, 10) else 1 for i in range(A)]
    acts = [STAY] * A
    for i in (2, 7, 10, 4, 6, 8):
        acts[i] = tag(i, 5)
    acts[3] = tag(3, 7)
    script += [dict(inject=dict(pos=spread, alive=dead, **fresh), actions=acts), stay]
    return script * 3  # (the drawn action orders differ between the repetitions)


def save_trace(name, spec, seed, env, arrs, notes):
    meta = dict(spec)
    meta.update(seed=int(seed), mode="given", notes=notes, metric_order=METRIC_ORDER, n_agents=int(env.n_agents), n_imposters=int(env.n_imposters),
                n_jobs=int(env.n_jobs), grid_used=np.asarray(env.grid, dtype=np.uint8).tolist(), imposter_idxs_final=[int(i) for i in env.imposter_idxs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrs)
    print(f"{name}: S={len(arrs['done'])} kills={int(arrs['metrics'][:, 0].max())} voted out={arrs['metrics'][-1, 1:3].tolist()} "
          f"max count={int(arrs['counts'].max())} size={os.path.getsize(path)} B")


def main():
    os.makedirs(OUT, exist_ok=True)
    spec = dict(**{"class": "tagging"}, kwargs=dict(n_imposters=2, n_crew=10, n_jobs=2, tag_reset_interval=2, vote_reward=3, shuffle_imposter_index=False,
                                                   is_action_order_random=True, include_walls=False))
    env, arrs = run_given(spec, 21, directed_script())
    save_trace("directed_tagging12_votes", spec, 21, env, arrs,
               "count 11 in word 2, 6/6 tie across words, tags around a kill, imposter voted out by 5..11, dead taggers / dead target")

    specs = {
        "tagging_1v8_j3_i5": dict(n_imposters=1, n_crew=8, n_jobs=3, tag_reset_interval=5),
        "tagging_2v9_j4_i7_tsr": dict(n_imposters=2, n_crew=9, n_jobs=4, tag_reset_interval=7, is_action_order_random=False, time_step_reward=-1, vote_reward=5),
        "tagging_3v9_j8_i4": dict(n_imposters=3, n_crew=9, n_jobs=8, tag_reset_interval=4, shuffle_imposter_index=True),
    }
    for name, kwargs in specs.items():
        spec = dict(**{"class": "tagging"}, kwargs=kwargs)
        crcs = np.zeros((N_SEEDS, N_STEPS), dtype=np.uint32)
        for seed in range(N_SEEDS):
            crcs[seed], env = run(spec, 1000 + seed)
        meta = dict(spec)
        meta.update(seeds=[1000 + s for s in range(N_SEEDS)], n_steps=N_STEPS, n_agents=int(env.n_agents), n_jobs=int(env.n_jobs),
                    n_imposters=int(env.n_imposters), grid_used=np.asarray(env.grid, dtype=np.uint8).tolist())
        np.savez_compressed(os.path.join(OUT, f"crc_{name}.npz"), meta=np.array(json.dumps(meta)), crc=crcs, crc_of_crcs=np.uint32(zlib.crc32(crcs.tobytes())))
        print(name, hex(zlib.crc32(crcs.tobytes())))


if __name__ == "__main__":
    main()
