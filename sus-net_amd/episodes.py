"""Per-episode returns and lengths of B environments in lockstep: the episode bookkeeping of the reference's ``train()``
(src/train.py:385-386 ``G = reward + gamma * G``; 419-438 ``G[imposter_mask].mean()``, ``G[~imposter_mask].mean()``, ``t_episode + 1``)
computed from the ``[T][B]`` feed block a collection leaves on the device (``DeviceReplayBuffer.last_feed``).

* HIP path (``susnet_episode_stats``, csrc/susnet_episodes.h): CUDA tensors; three launches per block, no host synchronisation, the
  log in device memory until ``records()``.
* numpy path: CPU tensors / arrays; the same rule in float64 with the same summation order, one tick at a time.

Log order is tick-major, env-minor on both paths: what a host loop over ticks and environments would append.

A feed that carries ``ep_info`` (``env.alloc_feed``: one ``susnet_episode_info`` per slot, written by the stepping kernels where an episode
ends) also fills a second log, parallel to the first: the ``info`` counters of every logged episode -- what the reference's
``metrics.step(info)`` appends at every episode end (src/train.py:419-427).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L

RECORD_DTYPE = np.dtype([("imposter_return", "<f8"), ("crew_return", "<f8"), ("tick", "<i8"), ("env", "<i4"), ("length", "<i4"),
                         ("ended_by", "<i4"), ("reserved", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(L.EpisodeRecord)
FIELDS = ("imposter_return", "crew_return", "length", "tick", "env", "ended_by")
# susnet_episode_info (include/susnet.h): 16 bytes, four int32 words in a feed tensor
INFO_DTYPE = np.dtype([("time_steps", "<u4"), ("completed_jobs", "<u4"), ("sabotaged_jobs", "<u4"), ("imp_killed_crew", "u1"),
                       ("imp_voted_out", "u1"), ("crew_voted_out", "u1"), ("outcome", "u1")])
assert INFO_DTYPE.itemsize == C.sizeof(L.EpisodeInfo) == 16
# records() name (the reference's SusMetrics value) <- record field; the two outcome flags come from `outcome`
INFO_FIELDS = {"imp_killed_crew": "imp_killed_crew", "imp_voted_out": "imp_voted_out", "crew_voted_out": "crew_voted_out",
               "sabotaged_jobs": "sabotaged_jobs", "completed_jobs": "completed_jobs", "total_time_steps": "time_steps"}
INFO_NAMES = tuple(INFO_FIELDS) + ("imposter_won", "crew_won")
MIN_AGENTS, MAX_AGENTS = 2, 12


def numpy_order_mean(values) -> float:
    """``np.asarray(values, float64).mean()`` for up to 12 values, spelled out: numpy's pairwise summation adds fewer than 8 values one
    by one from 0.0; from 8 values on it forms ``((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7))`` and adds the rest one by one.  Empty: NaN."""
    x = [float(v) for v in values]
    n = len(x)
    assert n <= MAX_AGENTS
    if n == 0:
        return float("nan")
    if n < 8:
        s = 0.0
        for v in x:
            s = s + v
    else:
        s = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))
        for v in x[8:]:
            s = s + v
    return s / n


def info_records(x) -> np.ndarray:
    """A feed's ``ep_info`` (``[T][B][4]`` int32 tensor / array, or an ``INFO_DTYPE`` array) as a host ``[T][B]`` array of ``INFO_DTYPE``."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype == INFO_DTYPE:
        return x
    if x.dtype.itemsize != 4 or x.shape[-1] != 4:
        raise ValueError(f"ep_info must be [T, B, 4] of 32-bit words or an array of INFO_DTYPE, got {x.dtype} {x.shape}")
    return np.ascontiguousarray(x).view(INFO_DTYPE).reshape(x.shape[:-1])


def pack_info(time_steps, completed_jobs, sabotaged_jobs, imp_killed_crew, imp_voted_out, crew_voted_out, imposter_won, crew_won) -> np.ndarray:
    """``INFO_DTYPE`` records from the counters of the reference's ``info`` dict (arrays of one shape): what the stepping kernels write."""
    out = np.zeros(np.shape(time_steps), dtype=INFO_DTYPE)
    out["time_steps"], out["completed_jobs"], out["sabotaged_jobs"] = time_steps, completed_jobs, sabotaged_jobs
    out["imp_killed_crew"] = np.minimum(imp_killed_crew, 255)
    out["imp_voted_out"], out["crew_voted_out"] = imp_voted_out, crew_voted_out
    out["outcome"] = (np.asarray(crew_won) != 0) * L.OUTCOME_CREW_WON + (np.asarray(imposter_won) != 0) * L.OUTCOME_IMPOSTER_WON
    return out


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype, copy=False)


class EpisodeLog:
    """Carry (``G`` per agent as float64, ``t_episode``), an append-only episode log of ``capacity`` records, and the ``count`` /
    ``dropped`` counters, for one batched env -- or, without an env (``n_agents=, batch=``), for CPU feed arrays.

    ``update(feed, n_ticks, tick_base)`` consumes the first ``n_ticks`` slots of a feed block (``rewards [T][B][A] float32``, ``done`` /
    ``truncated [T][B] bool``, ``roles [T][B] int16``: the imposter bitmask of the episode that acted; optionally ``ep_info [T][B][4]
    int32``: the ended episodes' ``susnet_episode_info``); ``records()`` returns the log as host arrays in log order -- with ``ep_info``
    feeds also the episodes' info counters (``INFO_NAMES``).  Episodes that find the log full are counted in ``dropped``.  A log takes
    feeds with ``ep_info`` or without, not a mixture."""

    def __init__(self, env=None, gamma: float = 0.99, capacity: int = 1 << 20, n_agents: Optional[int] = None, batch: Optional[int] = None,
                 device=None):
        self.env = env
        self.n_agents = int(env.n_agents if env is not None else n_agents)
        self.batch = int(env.batch if env is not None else batch)
        self.device = torch.device(env.device if env is not None else (device or "cpu"))
        self.gamma, self.capacity = float(gamma), int(capacity)
        if not MIN_AGENTS <= self.n_agents <= MAX_AGENTS:
            raise ValueError(f"EpisodeLog serves {MIN_AGENTS} .. {MAX_AGENTS} agents, got {self.n_agents}")
        if self.batch < 1 or self.capacity < 0:
            raise ValueError("EpisodeLog: batch must be positive, capacity non-negative")
        self.ticks = 0  # lockstep ticks consumed so far: the default tick_base of the next update
        self.has_info = None  # whether the feeds carry ep_info: fixed by the first update
        self._info_log = None  # the parallel log of susnet_episode_info records, allocated with the first ep_info feed
        if self.device.type == "cuda":
            if env is None:
                raise ValueError("EpisodeLog on a CUDA device needs the env whose feed it reads (the kernel takes its handle)")
            carry, ws = C.c_uint64(), C.c_uint64()
            L.check(env.lib.susnet_episode_stats_bytes(env._h, 1, C.byref(carry), C.byref(ws)))
            self._carry = torch.zeros(int(carry.value) // 4, dtype=torch.int32, device=self.device)
            self._counters = torch.zeros(2, dtype=torch.int64, device=self.device)  # [count, dropped]
            self._log = torch.zeros(max(self.capacity, 1) * RECORD_DTYPE.itemsize // 8, dtype=torch.int64, device=self.device)
            self._ws, self._ws_ticks = None, 0
        else:
            self._G = np.zeros((self.batch, self.n_agents), dtype=np.float64)
            self._t_episode = np.zeros(self.batch, dtype=np.int32)
            self._host_log = np.zeros(self.capacity, dtype=RECORD_DTYPE)
            self._count = self._dropped = 0

    # ---- state ----
    def reset(self, keep_log: bool = False) -> None:
        """Every environment at the start of an episode (after an ``env.reset()``); unless ``keep_log``, an empty log and zero counters."""
        if self.device.type == "cuda":
            self._carry.zero_()
            if not keep_log:
                self._counters.zero_()
        else:
            self._G[...] = 0.0
            self._t_episode[...] = 0
            if not keep_log:
                self._count = self._dropped = 0
        if not keep_log:
            self.ticks = 0
            self.has_info = None

    # ---- snapshot / restore ----
    def state_dict(self) -> dict:
        """The log between two ``update`` calls as host tensors and plain values, on both paths: the carry, the counters and the used part
        of the log and of the parallel info log (HIP path: ``_carry``, ``_counters``, ``_log``, ``_info_log``, copied to the host, which
        synchronises; numpy path: ``_G``, ``_t_episode``, ``_host_log``, ``_count``, ``_dropped``, the record arrays as their bytes), plus
        ``ticks`` and ``has_info``.  The workspace is scratch and is not saved."""
        sd = {"form": self.device.type, "n_agents": self.n_agents, "batch": self.batch, "gamma": self.gamma, "capacity": self.capacity,
              "ticks": int(self.ticks), "has_info": self.has_info}
        if self.device.type == "cuda":
            counters = self._counters.cpu()
            count = int(counters[0])
            sd.update(carry=self._carry.cpu(), counters=counters, log=self._log[:count * (RECORD_DTYPE.itemsize // 8)].cpu(),
                      info_log=None if self._info_log is None else self._info_log[:count].cpu())
        else:
            as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy())
            sd.update(G=torch.from_numpy(self._G.copy()), t_episode=torch.from_numpy(self._t_episode.copy()), count=int(self._count),
                      dropped=int(self._dropped), log=as_bytes(self._host_log[:self._count]),
                      info_log=None if self._info_log is None else as_bytes(self._info_log[:self._count]))
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Restore ``state_dict()``'s log into this one, built alike (form, agents, batch, gamma and capacity must agree: a difference is a
        ``ValueError`` that names it).  The next ``update`` continues the episodes in flight and appends behind the restored records."""
        mine = {"form": self.device.type, "n_agents": self.n_agents, "batch": self.batch, "gamma": self.gamma, "capacity": self.capacity}
        for k, v in mine.items():
            if sd[k] != v:
                raise ValueError(f"load_state_dict: the episode log was saved with {k} = {sd[k]!r}, this one has {v!r}")
        self.ticks, self.has_info = int(sd["ticks"]), sd["has_info"]
        info = sd["info_log"]
        if self.device.type == "cuda":
            self._carry.copy_(sd["carry"])
            self._counters.copy_(sd["counters"])
            self._log[:sd["log"].numel()].copy_(sd["log"])
            if info is None:
                self._info_log = None
            else:
                if self._info_log is None:
                    self._info_log = torch.zeros(max(self.capacity, 1), 4, dtype=torch.int32, device=self.device)
                self._info_log[:info.shape[0]].copy_(info)
        else:
            self._G[...] = sd["G"].numpy()
            self._t_episode[...] = sd["t_episode"].numpy()
            self._count, self._dropped = int(sd["count"]), int(sd["dropped"])
            self._host_log[:self._count] = sd["log"].numpy().view(RECORD_DTYPE)
            if info is None:
                self._info_log = None
            else:
                if self._info_log is None:
                    self._info_log = np.zeros(self.capacity, dtype=INFO_DTYPE)
                self._info_log[:self._count] = info.numpy().view(INFO_DTYPE)

    # ---- one feed block ----
    def update(self, feed: Dict[str, torch.Tensor], n_ticks: Optional[int] = None, tick_base: Optional[int] = None) -> None:
        n = int(feed["rewards"].shape[0] if n_ticks is None else n_ticks)
        base = self.ticks if tick_base is None else int(tick_base)
        if n < 1 or n > feed["rewards"].shape[0]:
            raise ValueError(f"EpisodeLog.update: n_ticks = {n} outside 1 .. {feed['rewards'].shape[0]}")
        if tuple(feed["rewards"].shape[1:]) != (self.batch, self.n_agents):
            raise ValueError(f"EpisodeLog.update: rewards {tuple(feed['rewards'].shape)} is not [T, {self.batch}, {self.n_agents}]")
        has_info = feed.get("ep_info") is not None
        if self.has_info is None:
            self.has_info = has_info
        elif self.has_info != has_info:
            raise ValueError("EpisodeLog.update: this log was started " + ("with" if self.has_info else "without") + " ep_info feeds; the two logs "
                             "must stay parallel")
        if self.device.type == "cuda":
            self._update_hip(feed, n, base)
        else:
            self._update_host(feed, n, base)
        self.ticks = base + n

    def _update_hip(self, feed, n, base):
        env = self.env
        rew, done, trunc, roles = feed["rewards"], feed["done"], feed["truncated"], feed["roles"]
        for name, t, dtypes in (("rewards", rew, (torch.float32,)), ("done", done, (torch.bool, torch.uint8)),
                                ("truncated", trunc, (torch.bool, torch.uint8)), ("roles", roles, (torch.int16,))):
            if t.dtype not in dtypes or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"EpisodeLog.update: {name} must be a contiguous {dtypes[0]} tensor on {self.device}")
            if name != "rewards" and tuple(t.shape) != tuple(rew.shape[:2]):
                raise ValueError(f"EpisodeLog.update: {name} {tuple(t.shape)} does not match rewards {tuple(rew.shape)}")
        if self._ws is None or self._ws_ticks < n:
            carry, ws = C.c_uint64(), C.c_uint64()
            L.check(env.lib.susnet_episode_stats_bytes(env._h, n, C.byref(carry), C.byref(ws)))
            self._ws, self._ws_ticks = torch.empty(int(ws.value) // 8 + 1, dtype=torch.int64, device=self.device), n
        io = L.EpisodeIO()
        io.n_ticks = n
        io.rewards, io.done, io.truncated, io.roles = rew.data_ptr(), done.data_ptr(), trunc.data_ptr(), roles.data_ptr()
        io.gamma, io.tick_base = self.gamma, base
        io.carry, io.carry_bytes = self._carry.data_ptr(), self._carry.numel() * 4
        io.log, io.capacity = self._log.data_ptr(), self.capacity
        io.count, io.dropped = self._counters.data_ptr(), self._counters.data_ptr() + 8
        io.workspace, io.workspace_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        if self.has_info:
            info = feed["ep_info"]
            if info.dtype != torch.int32 or not info.is_contiguous() or info.device != self.device or tuple(info.shape) != tuple(rew.shape[:2]) + (4,):
                raise ValueError(f"EpisodeLog.update: ep_info must be a contiguous int32 tensor [T, {self.batch}, 4] on {self.device}")
            if self._info_log is None:
                self._info_log = torch.zeros(max(self.capacity, 1), 4, dtype=torch.int32, device=self.device)
            io.info, io.info_log = info.data_ptr(), self._info_log.data_ptr()
        with torch.cuda.device(self.device):
            L.check(env.lib.susnet_episode_stats(env._h, C.byref(io), env._stream()))

    def _update_host(self, feed, n, base):
        rew = _host(feed["rewards"], np.float32)
        ended_by = (_host(feed["done"], bool).astype(np.int32) * L.EPISODE_DONE +
                    _host(feed["truncated"], bool).astype(np.int32) * L.EPISODE_TRUNCATED)
        roles = _host(feed["roles"], np.int16).astype(np.int64) & 0xFFFF
        gamma = np.float64(self.gamma)
        A = self.n_agents
        info = None
        if self.has_info:
            info = info_records(feed["ep_info"])
            if info.shape[1:] != (self.batch,) or info.shape[0] < n:
                raise ValueError(f"EpisodeLog.update: ep_info {info.shape} is not [T, {self.batch}] records")
            if self._info_log is None:
                self._info_log = np.zeros(self.capacity, dtype=INFO_DTYPE)
        for t in range(n):
            self._G = rew[t].astype(np.float64) + gamma * self._G  # train.py:386 (numpy rounds the product, then the sum)
            for b in np.flatnonzero(ended_by[t]):
                if self._count < self.capacity:
                    g, mask = self._G[b], int(roles[t, b])
                    rec = self._host_log[self._count]
                    rec["imposter_return"] = numpy_order_mean(g[a] for a in range(A) if (mask >> a) & 1)
                    rec["crew_return"] = numpy_order_mean(g[a] for a in range(A) if not (mask >> a) & 1)
                    rec["tick"], rec["env"], rec["length"], rec["ended_by"] = base + t, b, self._t_episode[b] + 1, ended_by[t, b]
                    if info is not None:
                        self._info_log[self._count] = info[t, b]
                    self._count += 1
                else:
                    self._dropped += 1
                self._G[b] = 0.0
                self._t_episode[b] = -1
            self._t_episode += 1

    # ---- reading the log (host synchronisation) ----
    def records(self) -> Dict[str, np.ndarray]:
        """The log in log order as host arrays ``imposter_return``, ``crew_return`` (float64), ``length``, ``tick``, ``env``, ``ended_by``,
        plus the scalars ``count`` and ``dropped``; a log fed with ``ep_info`` also returns the episodes' info counters under the reference's
        names (``INFO_NAMES``: ``imp_killed_crew``, ``imp_voted_out``, ``crew_voted_out``, ``sabotaged_jobs``, ``completed_jobs``,
        ``total_time_steps``, ``imposter_won``, ``crew_won``; int64).  Copies the used part of the log(s) to the host."""
        info = None
        if self.device.type == "cuda":
            count, dropped = (int(v) for v in self._counters.cpu())
            words = RECORD_DTYPE.itemsize // 8
            raw = self._log[:count * words].cpu().numpy().view(RECORD_DTYPE)
            if self.has_info:
                info = self._info_log[:count].cpu().numpy().view(INFO_DTYPE).reshape(count)
        else:
            count, dropped, raw = self._count, self._dropped, self._host_log[:self._count]
            if self.has_info:
                info = self._info_log[:count]
        out = {k: raw[k].copy() for k in FIELDS}
        if info is not None:
            for name, field in INFO_FIELDS.items():
                out[name] = info[field].astype(np.int64)
            out["imposter_won"] = ((info["outcome"] & L.OUTCOME_IMPOSTER_WON) != 0).astype(np.int64)
            out["crew_won"] = ((info["outcome"] & L.OUTCOME_CREW_WON) != 0).astype(np.int64)
        out["count"], out["dropped"] = count, dropped
        return out

    @property
    def counters(self):
        """Device ``int64[2]`` = ``[count, dropped]`` (HIP path), for callers that keep everything on the device."""
        return self._counters if self.device.type == "cuda" else torch.tensor([self._count, self._dropped])
