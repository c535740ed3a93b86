"""Shared by the tests of the SpatialDQN collection path: numpy restatements of the per-agent acting rule (susnet_agent_policy_actions)
and of the raw state window's push (susnet_state_window_push), and the reference trainer's own runs (tests/golden/spatial_collect/)."""
import glob
import os

import numpy as np
from conftest import GOLDEN_DIR, load_golden

SPATIAL_COLLECT_DIR = os.path.join(GOLDEN_DIR, "spatial_collect")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPATIAL_COLLECT_DIR, "*.npz")))
RING_FIELDS = ("states", "actions", "rewards", "next_states", "dones", "imposters")
MARGIN_FACTOR, KERNEL_TOLERANCE = 100.0, 2e-5
SIZE_CAP = 1 << 20


def load_case(name):
    return load_golden(os.path.join(SPATIAL_COLLECT_DIR, name + ".npz"))


def first_argmax(q):
    """Index of the first maximum of every row of ``q[..., n]`` by the kernel's own rule: start at 0, move on ``v > best`` only (so of
    +0.0 and -0.0, equal under ``>``, the earlier one wins, as in np.argmax / torch.argmax)."""
    q = np.asarray(q, dtype=np.float32)
    best = np.zeros(q.shape[:-1], dtype=np.int64)
    hi = q[..., 0].copy()
    for k in range(1, q.shape[-1]):
        better = q[..., k] > hi
        best = np.where(better, k, best)
        hi = np.where(better, q[..., k], hi)
    return best


def agent_actions_reference(q_imposter, q_crew, imposter_mask, alive, mask_dead=True, sampled=None, explore=None):
    """train.py:351-381 for ``[B, A]`` agents with one Q row each: agent (b, i) takes the first argmax of ``q_imposter[b, i]`` if it is an
    imposter of env b, else of ``q_crew[b, i]`` (``q_crew`` None: its ``sampled`` index); where ``explore`` its ``sampled`` index instead;
    dead agents 0 when ``mask_dead``."""
    imposter_mask, alive = np.asarray(imposter_mask).astype(bool), np.asarray(alive).astype(bool)
    crew = first_argmax(q_crew) if q_crew is not None else np.asarray(sampled).astype(np.int64)
    a = np.where(imposter_mask, first_argmax(q_imposter), crew)
    if explore is not None:
        a = np.where(np.asarray(explore).astype(bool), np.asarray(sampled).astype(np.int64), a)
    if mask_dead:
        a = np.where(alive, a, 0)
    return a.astype(np.int64)


def state_window_push_reference(window, obs, ended):
    """train.py:388-389 / 441-445 for ``window [B, T, S]``: where ``ended`` the new state ``obs [B, S]`` T times, else the window shifted by
    one with ``obs`` in the last slot.  Returns a new array."""
    window, obs = np.asarray(window), np.asarray(obs)
    T = window.shape[1]
    nxt = np.roll(window, -1, axis=1)
    nxt[:, -1] = obs
    full = np.repeat(obs[:, None, :], T, axis=1)
    return np.where(np.asarray(ended).astype(bool)[:, None, None], full, nxt)
