"""Shared by the tests of the dense learner's sweep step (susnet_mlp_train_sweep): learners whose complete susnet_mlp_train_io is made by
hand as tests/train_exact.py's abi_step makes it -- canaries around every buffer the call writes and behind the workspace -- kept alive
over several calls, so the same learner can take its own susnet_mlp_train_step or stand in a sweep call; a learner and its twin are built
from the same seeds.  Importing this module touches no GPU: device buffers are made inside the functions the GPU tests call."""
import ctypes as C

import numpy as np
import torch

from train_exact import BETAS, CANARY, DEV, _team_buffers, _workspace, n_params

GAMMAS, LRS = (0.99, 0.9, 0.8), (1e-3, 3e-4, 1e-2)
# the grid's documented constants (csrc/susnet_mlp_train.h): workgroups of the gradient kernel, and all workgroups' partials together
MAX_GRID, MAX_PARTIAL_BYTES, TILE = 256, 64 << 20, 32


def documented_grid(dims_pair, n):
    """G = min(kMtMaxGrid, tiles of n, kMtMaxPartialBytes / (4 Pp)) workgroups, at least 1 (Pp: the widest enabled team's P + 1, rounded up
    to 4) -- the header's formula, restated; -> (G, tiles of n)."""
    pp = max((n_params(d) + 1 + 3) // 4 * 4 for d in dims_pair if d is not None)
    tiles = (n + TILE - 1) // TILE
    return max(1, min(MAX_GRID, tiles, MAX_PARTIAL_BYTES // (4 * pp))), tiles


def make_batch(rng, F, n_out, n, A=4, M=None, imposter_agents=None, all_done=False):
    """A batch as abi_step takes it: float feature rows, n sampled rows of a ring of M, the imposter drawn from `imposter_agents`."""
    M = n + 5 if M is None else M
    agents = np.arange(A) if imposter_agents is None else np.asarray(imposter_agents)
    return dict(feat=(rng.random((n, F)).round(3) * (rng.random((n, F)) < 0.5)).astype(np.float32),
                next_feat=(rng.random((n, F)).round(3) * (rng.random((n, F)) < 0.5)).astype(np.float32),
                idx=rng.integers(0, M, n).astype(np.int64), actions=rng.integers(0, n_out, (M, A)), rewards=rng.normal(size=(M, A)).astype(np.float32),
                dones=np.ones(M, dtype=np.uint8) if all_done else (rng.random(M) < 0.3).astype(np.uint8),
                imposters=agents[rng.integers(0, len(agents), M)].astype(np.int16))


def make_teams(rng, dims_pair, lr):
    """Per team None or abi_step's dict: random float weights (fan-in scaled), a target network of its own."""
    out = []
    for dims in dims_pair:
        if dims is None:
            out.append(None)
            continue

        def flat():  # MLP.parameters() order: W0, b0, a0, W1, b1, a1, ..., W_last, b_last
            parts = []
            for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
                parts += [rng.normal(0, 1 / np.sqrt(a), a * b), rng.normal(0, 0.1, b)]
                if l < len(dims) - 2:
                    parts.append(np.asarray([0.25]))
            return np.concatenate(parts).astype(np.float32)

        out.append(dict(dims=list(dims), params=flat(), target=flat(), lr=lr, betas=BETAS))
    return out


class Learner:
    """One learner's complete call, kept alive: the batch on the device, the teams' guarded buffers, losses between canaries, its workspace."""

    def __init__(self, pkg, env, teams, batch, gamma, losses_fill=0.0):
        L = pkg._lib
        self.pkg, self.env, self.teams = pkg, env, teams
        io = self.io = L.MlpTrainIO()
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
        n = len(batch["idx"])
        self.tensors = dict(feat=dev(batch["feat"], torch.float32), next_feat=dev(batch["next_feat"], torch.float32), idx=dev(batch["idx"], torch.int64),
                            actions=dev(batch["actions"], torch.int64), rewards=dev(batch["rewards"], torch.float32), dones=dev(batch["dones"], torch.uint8),
                            imposters=dev(batch["imposters"].reshape(-1, 1), torch.int16))
        t = self.tensors
        if n > 0:
            io.feat, io.next_feat, io.indices = t["feat"].data_ptr(), t["next_feat"].data_ptr(), t["idx"].data_ptr()
        io.n = n
        io.actions, io.rewards, io.dones, io.imposters = t["actions"].data_ptr(), t["rewards"].data_ptr(), t["dones"].data_ptr(), t["imposters"].data_ptr()
        io.max_size, io.gamma = t["actions"].shape[0], gamma
        self.bufs = [None if tm is None else _team_buffers(io.team[k], tm) for k, tm in enumerate(teams)]
        self.losses = torch.full((4,), CANARY, dtype=torch.float32, device=DEV)  # [canary, imposter, crew, canary]
        self.losses[1:3] = losses_fill
        io.losses_out = self.losses.data_ptr() + 4
        nbytes = C.c_uint64()
        L.check(env.lib.susnet_mlp_train_workspace_bytes(env._h, C.byref(io), C.byref(nbytes)))
        self.ws_bytes = int(nbytes.value)
        self.ws = _workspace(self.ws_bytes)
        io.workspace, io.workspace_bytes = self.ws.data_ptr(), self.ws_bytes

    def step(self):
        """The learner's own susnet_mlp_train_step."""
        with torch.cuda.device(DEV):
            self.pkg._lib.check(self.env.lib.susnet_mlp_train_step(self.env._h, C.byref(self.io), self.env._stream()))

    def written(self):
        """Everything the call may write, as int32 views (bit patterns): losses, and per enabled team params, exp_avg, exp_avg_sq, step."""
        out = [("losses", self.losses[1:3])]
        for t, g in enumerate(self.bufs):
            if g is not None:
                out += [(f"team {t} {k}", g[k].view) for k in ("params", "exp_avg", "exp_avg_sq")] + [(f"team {t} step", g["step"])]
        return [(name, x.view(torch.int32)) for name, x in out]

    def snapshot(self):
        return [x.clone() for _, x in self.written()]

    def restore(self, saved):
        for (_, x), s in zip(self.written(), saved):
            x.copy_(s)

    def steps(self):
        return [None if g is None else float(g["step"]) for g in self.bufs]

    def check_canaries(self):
        lo = self.losses.cpu().numpy()
        assert lo[0] == CANARY and lo[3] == CANARY, "losses_out: a neighbour was written"
        assert bool((self.ws[self.ws_bytes:] == 0x5A).all()), "the workspace was overrun"
        for t, g in enumerate(self.bufs):
            if g is None:
                continue
            for k in ("params", "target", "exp_avg", "exp_avg_sq"):
                assert g[k].intact(), f"team {t} {k}: a canary was overwritten"
            assert np.array_equal(g["target"].view.cpu().numpy(), np.asarray(self.teams[t]["target"], dtype=np.float32)), "the target network was written"


def sweep_call(pkg, learners, K=None):
    """One susnet_mlp_train_sweep over `learners`; -> the return code (the caller checks it)."""
    L = pkg._lib
    n = len(learners)
    ios = (L.MlpTrainIO * n)(*[l.io for l in learners])
    envs = (C.c_void_p * n)(*[l.env._h for l in learners])
    env = learners[0].env
    with torch.cuda.device(DEV):
        return env.lib.susnet_mlp_train_sweep(envs, ios, n if K is None else K, env._stream())


def sweep_step(pkg, learners):
    pkg._lib.check(sweep_call(pkg, learners))


def assert_same(a, b, what):
    """Learner `a` and its twin `b`: every written buffer bit for bit."""
    for (name, x), (_, y) in zip(a.written(), b.written()):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} words"


def build(pkg, env, K, dims_pair, n, seed, twins=2, **batch_kw):
    """`twins` sets of K learners from the same seeds: learner k has its own weights, batch, indices, gamma and learning rate.  batch_kw:
    make_batch's, or per learner through `per_learner` = {k: kwargs}."""
    per = batch_kw.pop("per_learner", {})
    first = next(d for d in dims_pair if d is not None)
    n_out = min(d[-1] for d in dims_pair if d is not None)
    out = []
    for _ in range(twins):
        members = []
        for k in range(K):
            rng = np.random.default_rng(1000 * seed + k)
            batch = make_batch(rng, first[0], n_out, n, **dict(batch_kw, **per.get(k, {})))
            members.append(Learner(pkg, env, make_teams(rng, dims_pair, LRS[k % 3]), batch, GAMMAS[k % 3]))
        out.append(members)
    return out
