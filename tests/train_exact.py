"""Shared by the exact tests of the two device train steps (susnet_dqn_train_step, the fused learner of the compiled-in layouts, and
susnet_mlp_train_step, the dense one): a float64 restatement of DQNTeamTrainer.train_step that records, for every sum it takes, whether
ANY float32 summation order reproduces it (ExactSums); integer networks; batches on the directed states of tests/qnet_exact.py with
their feature rows from the CPU oracle; float64 Adam; and the two C-ABI calls made by hand with canaries around every buffer they
write.  Used by test_train_exact_host.py (CPU: the restatement against float64 autograd, the cases' exactness and coverage),
test_gpu_train_exact.py and test_gpu_mlp_train.py.  Importing this module touches no GPU: device buffers are made inside the functions
the GPU tests call."""
import ctypes as C
import math

import numpy as np
import torch

import qnet_exact as X

DEV = "cuda:0"
CANARY = 12345.0
BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults (train.py:24-38)


# ---- flat parameter buffers ---------------------------------------------------------------------------------------------------------------
def n_params(dims):
    return sum(a * b + b for a, b in zip(dims[:-1], dims[1:])) + len(dims) - 2


def flatten(W, B, slopes):
    """MLP.parameters() order: W0, b0, a0, W1, b1, a1, ..., W_last, b_last."""
    parts = []
    for l, (w, b) in enumerate(zip(W, B)):
        parts += [np.asarray(w).reshape(-1), np.asarray(b).reshape(-1)]
        if l < len(W) - 1:
            parts.append(np.asarray([slopes[l]]))
    return np.concatenate(parts)


def split(dims, flat):
    """-> [(name, array)] per tensor of a flat parameter-order buffer."""
    out, off = [], 0
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        out.append((f"W{l}", flat[off:off + a * b].reshape(b, a)))
        off += a * b
        out.append((f"b{l}", flat[off:off + b]))
        off += b
        if l < len(dims) - 2:
            out.append((f"a{l}", flat[off:off + 1]))
            off += 1
    assert off == len(flat)
    return out


class Guarded:
    """A float32 device buffer of `n` values with canaries in front and behind, `lead` floats into its allocation: lead = 1 (the
    default) puts it at an ODD 4-byte offset, lead = 4 keeps the 16-byte alignment a packed image needs.  `fill`: the initial value
    where no `values` are given."""

    def __init__(self, values=None, n=None, lead=1, fill=0.0):
        n = len(values) if values is not None else n
        self.n, self.lead = n, lead
        self.buf = torch.full((n + lead + 3,), CANARY, dtype=torch.float32, device=DEV)
        self.view = self.buf[lead:lead + n]
        self.view.copy_(torch.as_tensor(np.asarray(values, dtype=np.float32)) if values is not None else torch.full((n,), fill))
        assert self.view.data_ptr() % 16 == (4 * lead) % 16

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        return self.view.cpu().numpy().astype(np.float64)

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lead] == CANARY).all()) and bool((b[self.lead + self.n:] == CANARY).all())


# ---- the exactness condition --------------------------------------------------------------------------------------------------------------
class ExactSums:
    """Collects, for every sum of the restatement, the condition under which EVERY summation order is exact in float32: all terms are
    multiples of one power of two q and sum |term| / q < 2^24 (every partial sum is then a multiple of q below 2^24 q)."""

    def __init__(self):
        self.worst, self.ok = 0.0, True

    @staticmethod
    def quantum(x):
        """The largest power of two that divides every entry of x (float64), or inf for all zeros."""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        x = x[x != 0]
        if x.size == 0:
            return math.inf
        m, e = np.frexp(x)
        mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
        low = mi & -mi  # lowest set bit of the 53-bit mantissa
        return float(2.0 ** (np.min(e.astype(np.float64) + np.log2(low.astype(np.float64))) - 53))

    @classmethod
    def quantum_cols(cls, x):
        """quantum() of every column of a matrix."""
        return np.array([cls.quantum(x[:, j]) for j in range(x.shape[1])])

    def check(self, q, abs_sums):
        """One family of sums: the per-sum totals of |term| and the quantum of each sum's terms (one for the family, or one per sum)."""
        abs_sums = np.asarray(abs_sums, dtype=np.float64)
        q = np.broadcast_to(np.asarray(q, dtype=np.float64), abs_sums.shape)
        live = np.isfinite(q) & (abs_sums > 0)  # (a sum of zeros is exact)
        if not live.any():
            return True
        ratio = float(np.max(abs_sums[live] / q[live]))
        self.worst = max(self.worst, ratio)
        good = ratio < 2.0 ** 24
        self.ok = self.ok and good
        return good

    def matmul(self, a, b, extra=None):
        """sum_k a[i, k] b[k, j] (+ extra[j]): terms are multiples of q(a) q(b)."""
        q = self.quantum(a) * self.quantum(b)
        tot = np.abs(a) @ np.abs(b)
        if extra is not None:
            q = min(q, self.quantum(extra))
            tot = tot + np.abs(extra)
        return self.check(q, tot)

    def log2_worst(self):
        return math.log2(max(self.worst, 1.0))


def exact_net(rng, dims, nnz=4):
    """Every unit: `nnz` nonzero +-1 inputs (all of them where the layer is narrower), bias in {-1, 0, 1}."""
    W, B = [], []
    for a, b in zip(dims[:-1], dims[1:]):
        w = np.zeros((b, a))
        for u in range(b):
            cols = rng.choice(a, size=min(nnz, a), replace=False)
            w[u, cols] = rng.choice([-1.0, 1.0], size=len(cols))
        W.append(w)
        B.append(rng.integers(-1, 2, b).astype(np.float64))
    return W, B


# ---- the float64 restatement of the train step ---------------------------------------------------------------------------------------------
def np_forward(W, B, X_, slope=0.5, ex=None):
    Z, h = [], X_
    for l in range(len(W)):
        if ex is not None:
            ex.matmul(h, W[l].T, B[l])
        z = h @ W[l].T + B[l]
        Z.append(z)
        h = np.where(z > 0, z, slope * z)
    return Z


def np_train_step(dims, online, target, batch, agents_rows, gamma, ex, slope=0.5):
    """The float64 restatement of one team's updates with lr = 0 (the weights never move): the gradient accumulated over `agents_rows`
    = [(agent, batch positions)], flat in parameter order, the summed losses, the number of non-empty updates, whether every update's
    loss sum met the exactness condition (its mean is then a float32 value), and a dict: `loss32`, the updates' means accumulated in
    float32 in update order -- what the step reports where the loss sums are exact, the rounding of each `losses[team] +=` included --
    and `updates`, the non-empty updates' own gradient totals (flat) in update order: Adam steps once per update, on the sum of the
    totals so far (train.py:64-67).  The gradient's sums are recorded in `ex` as the step defines them: within ONE update every word is
    one sum over the list's rows (any order: tiles, workgroups, lanes), and the updates' gradients then accumulate in agent order
    (zero_grad once per call) -- a second sum whose terms are the updates' totals."""
    W, B = online
    L_ = len(W)
    gW, gB, gA = [np.zeros_like(w) for w in W], [np.zeros_like(b) for b in B], [0.0] * (L_ - 1)
    aW, aB, aA = [np.zeros_like(w) for w in W], [np.zeros_like(b) for b in B], [0.0] * (L_ - 1)  # sums over updates of |update's total|
    qW, qB, qA = [np.full(w.shape, math.inf) for w in W], [np.full(b.shape, math.inf) for b in B], [math.inf] * (L_ - 1)  # quanta of the totals
    loss_total, loss32, steps, loss_exact, updates = 0.0, np.float32(0.0), 0, True, []
    for agent, rows in agents_rows:
        cnt = len(rows)
        if cnt == 0:
            continue
        steps += 1
        r = batch["idx"][rows]
        Xs, Xn = batch["feat"][rows], batch["next_feat"][rows]
        qn = np_forward(*target, Xn, slope, ex)[-1]
        rew = batch["rewards"][r, agent].astype(np.float64)
        y = np.where(batch["dones"][r] != 0, rew, rew + gamma * qn.max(1))
        Z = np_forward(W, B, Xs, slope, ex)
        act = batch["actions"][r, agent]
        diff = Z[-1][np.arange(cnt), act] - y
        ex.check(min(ex.quantum(Z[-1]), ex.quantum(y)), np.abs(Z[-1][np.arange(cnt), act]) + np.abs(y))
        sq = diff * diff
        loss_ex = ExactSums()
        loss_ex.check(loss_ex.quantum(sq), np.array([sq.sum()]))
        loss_exact = loss_exact and loss_ex.ok and float(np.float32(sq.sum() / cnt)) == sq.sum() / cnt
        loss_total += sq.sum() / cnt
        loss32 = np.float32(loss32 + np.float32(sq.sum() / cnt))
        dz = np.zeros_like(Z[-1])
        dz[np.arange(cnt), act] = 2.0 / cnt * diff
        uWs, uBs, uAs = [None] * L_, [None] * L_, [0.0] * (L_ - 1)
        for l in range(L_ - 1, -1, -1):
            h = Xs if l == 0 else np.where(Z[l - 1] > 0, Z[l - 1], slope * Z[l - 1])
            q_w = np.outer(ex.quantum_cols(dz), ex.quantum_cols(h))  # dW[n][k]: terms dz[s][n] h[s][k]
            ex.check(q_w, np.abs(dz).T @ np.abs(h))
            ex.check(ex.quantum_cols(dz), np.abs(dz).sum(0))
            uW, uB = dz.T @ h, dz.sum(0)
            uWs[l], uBs[l] = uW, uB
            gW[l], aW[l], qW[l] = gW[l] + uW, aW[l] + np.abs(uW), np.minimum(qW[l], q_w)
            gB[l], aB[l], qB[l] = gB[l] + uB, aB[l] + np.abs(uB), np.minimum(qB[l], ex.quantum_cols(dz))
            if l > 0:
                ex.matmul(dz, W[l])
                dh = dz @ W[l]
                z = Z[l - 1]
                terms = np.where(z > 0, 0.0, z * dh)
                ex.check(ex.quantum(terms), np.array([np.abs(terms).sum()]))
                uAs[l - 1] = terms.sum()
                gA[l - 1], aA[l - 1], qA[l - 1] = gA[l - 1] + terms.sum(), aA[l - 1] + abs(terms.sum()), min(qA[l - 1], ex.quantum(terms))
                dz = np.where(z > 0, dh, slope * dh)
        updates.append(flatten(uWs, uBs, uAs))
    for l in range(L_):  # the accumulation over the updates
        ex.check(qW[l], aW[l])
        ex.check(qB[l], aB[l])
        if l < L_ - 1:
            ex.check(qA[l], np.array([aA[l]]))
    return flatten(gW, gB, gA), loss_total, steps, loss_exact, dict(loss32=float(loss32), updates=updates)


# ---- float64 Adam -------------------------------------------------------------------------------------------------------------------------
def adam_f64(p, m, v, step, grads, lr, betas, eps):
    """torch.optim.Adam (single-tensor form, no weight decay, no amsgrad) in float64: one step per entry of `grads`, each the gradient
    ACCUMULATED so far in its call.  -> (p, m, v, step)."""
    p, m, v = (np.array(x, dtype=np.float64) for x in (p, m, v))
    for g in grads:
        step += 1
        m = m + (1.0 - betas[0]) * (g - m)
        v = betas[1] * v + (1.0 - betas[1]) * g * g
        bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
        p = p - lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v, step


# ---- torch_train_step on CPU modules ------------------------------------------------------------------------------------------------------
def mlp_of(pkg, dims, flat, dtype=torch.float64):
    """pkg.MLP(dims) in `dtype` holding the flat parameter-order values."""
    with torch.random.fork_rng(devices=[]):
        m = pkg.MLP(list(dims)).to(dtype)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.as_tensor(np.asarray(flat[off:off + p.numel()], dtype=np.float64)).to(dtype).view_as(p))
            off += p.numel()
    assert off == len(flat)
    return m


def torch_step(pkg, dims_pair, params, targets, batch, gamma, lr, betas, eps, dtype=torch.float64):
    """pkg.torch_train_step (DQNTeamTrainer.train_step, train.py:50-149) on CPU modules of `dtype` fed the batch's feature rows; a team
    of dims None does not train.  -> (losses [2], per team the flat exp_avg, exp_avg_sq, parameters after the call (None: untrained),
    per team the step count)."""
    A = batch["actions"].shape[1]
    ms = [mlp_of(pkg, d, p, dtype) if d is not None else None for d, p in zip(dims_pair, params)]
    ts = [mlp_of(pkg, d, p, dtype) if d is not None else None for d, p in zip(dims_pair, targets)]
    opts = [torch.optim.Adam(m.parameters(), lr=lr, betas=betas, eps=eps) if m is not None else None for m in ms]
    idx = torch.as_tensor(batch["idx"])
    z = torch.zeros(len(idx), 1, 1, dtype=dtype)
    fs, fn = (torch.as_tensor(np.asarray(batch[k], dtype=np.float64)).to(dtype).unsqueeze(1) for k in ("feat", "next_feat"))
    losses = pkg.torch_train_step(ms, ts, opts, gamma, [(z, fs)] * A, [(z, fn)] * A, torch.as_tensor(batch["actions"])[idx].long(),
                                  torch.as_tensor(np.asarray(batch["rewards"], dtype=np.float64))[idx].to(dtype),
                                  torch.as_tensor(batch["dones"])[idx].bool().reshape(-1, 1),
                                  torch.as_tensor(batch["imposters"])[idx].to(torch.int16).reshape(-1, 1))
    ea, eas, prm, steps = [], [], [], []
    for m, o in zip(ms, opts):
        if m is None:
            ea.append(None), eas.append(None), prm.append(None), steps.append(0.0)
            continue
        state = lambda key: np.concatenate([(o.state[p][key].double().numpy().reshape(-1) if p in o.state else np.zeros(p.numel())) for p in m.parameters()])
        ea.append(state("exp_avg")), eas.append(state("exp_avg_sq"))
        prm.append(np.concatenate([p.detach().double().numpy().reshape(-1) for p in m.parameters()]))
        steps.append(float(next(iter(o.state.values()))["step"]) if o.state else 0.0)
    return np.asarray(losses, dtype=np.float64), ea, eas, prm, steps


# ---- batches on the directed states -------------------------------------------------------------------------------------------------------
JOB_FILL = 99.0  # the ring rows' job fields: a value no grid holds -- tr_build_x must not read them


def state_size(layout):
    """flattened_state_size of the layout's game (base.py:230-235): positions, alive flags, job positions, job flags."""
    lay = X.LAYOUTS[layout]
    return 3 * lay["A"] + 3 * (0 if lay["game"] == "itg" else 4)


def ring_rows(layout, states, S):
    """Flattened ring rows [x0, y0, .., alive.., rest] (base.py:234-235) of directed states, float32 [n, S]; the trailing job fields
    hold JOB_FILL."""
    A = X.LAYOUTS[layout]["A"]
    n = len(states["pos"])
    assert S >= 3 * A
    rows = np.full((n, S), JOB_FILL, dtype=np.float32)
    rows[:, :2 * A] = states["pos"].reshape(n, 2 * A)
    rows[:, 2 * A:3 * A] = states["alive"]
    return rows


def is_pow2(c):
    return c > 0 and c & (c - 1) == 0


def team_lists(imposters_at, A):
    """Per team [(agent, batch positions)] in the step's order: the imposter team's rows of agent a are those whose imposter is a."""
    pos = np.arange(len(imposters_at))
    return [[(a, pos[imposters_at == a]) for a in range(A)], [(a, pos[imposters_at != a]) for a in range(A)]]


def fused_case(layout, dims, n, counts, seed, slope=0.5, gamma=0.5, nnz=4):
    """One susnet_dqn_train_step call on a ring of M = n + 7 rows of the layout's directed states, integer networks and dyadic
    constants.  dims: one stack for both teams or (imposter stack, crew stack); counts[a]: on how many SAMPLED rows agent a is the
    imposter (sum = n).  States and next states are drawn from all N_STATES directed states, the unplayable ones included; `idx` is a
    shuffled draw in which ring rows repeat (an eighth of each agent's rows, as far as every list keeps enough distinct rows to take
    every action); about a quarter of the ring rows are done rows; rewards are integers in [-3, 3]; within every (agent, team) list
    the actions walk through every output.  Every non-empty list has a power-of-two count (asserted): 2 / count is dyadic.
    -> dict(batch = np_train_step's form with the oracle's feature rows, nets = per team ((W, B) online, (W, B) target), lists = per
    team [(agent, batch positions)], ring = the ring tensors, dims = per team, layout, slope, gamma, state_index / next_index = the
    directed state of every ring row)."""
    lay = X.LAYOUTS[layout]
    A, F = lay["A"], lay["F"]
    dims_pair = [list(d) for d in dims] if isinstance(dims[0], (list, tuple)) else [list(dims), list(dims)]
    assert all(len(d) == 6 and d[0] == F for d in dims_pair) and len(counts) == A and sum(counts) == n
    rng = np.random.default_rng(seed)
    M = n + 7
    n_out = [d[-1] for d in dims_pair]
    # the sampled positions, grouped by imposter: distinct ring rows, then repeats of rows of the same group
    free = list(rng.permutation(M))
    idx, who = [], []
    for a, c in enumerate(counts):
        if c == 0:
            continue
        rep = min(c // 8, max(0, c - max(n_out)))
        own = [int(free.pop()) for _ in range(c - rep)]
        idx += own + [own[int(k)] for k in rng.integers(0, len(own), rep)]
        who += [a] * c
    order = rng.permutation(n)
    idx, who = np.array(idx, dtype=np.int64)[order], np.array(who, dtype=np.int16)[order]
    imposters = rng.integers(0, A, M).astype(np.int16)  # (rows outside the batch: anybody)
    imposters[idx] = who
    assert all(int((imposters[idx] == a).sum()) == c for a, c in enumerate(counts))
    lists = team_lists(imposters[idx], A)
    for t in range(2):
        assert all(len(r) == 0 or is_pow2(len(r)) for _, r in lists[t]), "2 / count must be dyadic"
    actions = np.zeros((M, A), dtype=np.int64)
    for t in range(2):
        for a, rows in lists[t]:
            distinct = np.unique(idx[rows])
            actions[distinct, a] = rng.permutation(len(distinct)) % n_out[t]
    for a in range(A):  # rows outside the batch: any valid action
        rest = np.setdiff1d(np.arange(M), idx)
        actions[rest, a] = rng.integers(0, min(n_out), len(rest))
    state_index, next_index = rng.integers(0, X.N_STATES, M), rng.integers(0, X.N_STATES, M)
    st, rows = X.directed_states(layout), X.oracle_rows(layout)
    S = state_size(layout)
    pick = lambda which: {k: st[k][which] for k in ("pos", "alive", "imp")}
    ring = dict(states=ring_rows(layout, pick(state_index), S), next_states=ring_rows(layout, pick(next_index), S))
    batch = dict(feat=rows[state_index[idx]].astype(np.float64), next_feat=rows[next_index[idx]].astype(np.float64), idx=idx, actions=actions,
                 rewards=rng.integers(-3, 4, (M, A)).astype(np.float64), dones=(rng.random(M) < 0.25).astype(np.uint8), imposters=imposters)
    nets = [(exact_net(rng, dims_pair[t], nnz), exact_net(rng, dims_pair[t], nnz)) for t in range(2)]
    return dict(batch=batch, nets=nets, lists=lists, ring=ring, dims=dims_pair, layout=layout, slope=slope, gamma=gamma, state_index=state_index,
                next_index=next_index, n=n, counts=tuple(counts), enabled=(True, True))


def float_case(layout, n, seed):
    """A batch of n rows with RANDOM imposters and float rewards on the layout's directed states (ring of n + 5 rows, indices drawn
    with replacement): the ragged-count cases.  The same dict as fused_case, without nets."""
    lay = X.LAYOUTS[layout]
    A = lay["A"]
    rng = np.random.default_rng(seed)
    M = n + 5
    idx = rng.integers(0, M, n).astype(np.int64)
    imposters = rng.integers(0, A, M).astype(np.int16)
    state_index, next_index = rng.integers(0, X.N_STATES, M), rng.integers(0, X.N_STATES, M)
    st, rows = X.directed_states(layout), X.oracle_rows(layout)
    S = state_size(layout)
    pick = lambda which: {k: st[k][which] for k in ("pos", "alive", "imp")}
    ring = dict(states=ring_rows(layout, pick(state_index), S), next_states=ring_rows(layout, pick(next_index), S))
    batch = dict(feat=rows[state_index[idx]], next_feat=rows[next_index[idx]], idx=idx, actions=rng.integers(0, lay["n_crew"], (M, A)),
                 rewards=rng.normal(size=(M, A)).astype(np.float32), dones=(rng.random(M) < 0.3).astype(np.uint8), imposters=imposters)
    return dict(batch=batch, lists=team_lists(imposters[idx], A), ring=ring, layout=layout, n=n)


def case_reference(case, ex=None):
    """np_train_step of the enabled teams of a fused_case: (ExactSums, [team 0's results or None, team 1's])."""
    ex = ExactSums() if ex is None else ex
    want = [np_train_step(case["dims"][t], case["nets"][t][0], case["nets"][t][1], case["batch"], case["lists"][t], case["gamma"], ex, case["slope"])
            if case["enabled"][t] else None for t in range(2)]
    return ex, want


def case_teams(case, lr=0.0, betas=(0.0, 0.999), eps=EPS):
    """The `teams` argument of fused_abi_step / abi_step for a fused_case: flat integer parameters, every slope = the case's; None for a team the case leaves out."""
    slopes = [case["slope"]] * 4
    return [dict(dims=case["dims"][t], params=flatten(*case["nets"][t][0], slopes), target=flatten(*case["nets"][t][1], slopes), lr=lr, betas=betas,
                 eps=eps) if case["enabled"][t] else None for t in range(2)]


# ---- the two C-ABI calls by hand ----------------------------------------------------------------------------------------------------------
def _team_buffers(io_team, tm):
    """Guarded params / target / exp_avg / exp_avg_sq and the step word of one team, written into its susnet_dqn_team.  tm: dict(dims,
    params, target, lr, betas[, eps, exp_avg, exp_avg_sq, step]) -- the optional entries carry Adam state from an earlier call."""
    P = n_params(tm["dims"])
    assert len(tm["params"]) == P == len(tm["target"])
    g = dict(params=Guarded(tm["params"]), target=Guarded(tm["target"]),
             exp_avg=Guarded(tm["exp_avg"]) if tm.get("exp_avg") is not None else Guarded(n=P),
             exp_avg_sq=Guarded(tm["exp_avg_sq"]) if tm.get("exp_avg_sq") is not None else Guarded(n=P),
             step=torch.full((1,), float(tm.get("step", 0.0)), dtype=torch.float32, device=DEV))
    io_team.enabled, io_team.n_dims = 1, len(tm["dims"])
    for k, d in enumerate(tm["dims"]):
        io_team.dims[k] = d
    io_team.lr, io_team.beta1, io_team.beta2, io_team.eps = tm["lr"], tm["betas"][0], tm["betas"][1], tm.get("eps", EPS)
    io_team.params, io_team.target_params = g["params"].ptr(), g["target"].ptr()
    io_team.exp_avg, io_team.exp_avg_sq, io_team.step = g["exp_avg"].ptr(), g["exp_avg_sq"].ptr(), g["step"].data_ptr()
    return g


def _team_results(bufs, teams):
    out = [None, None]
    for t, g in enumerate(bufs):
        if g is None:
            continue
        for k in ("params", "target", "exp_avg", "exp_avg_sq"):
            assert g[k].intact(), f"team {t} {k}: a canary was overwritten"
        assert np.array_equal(g["target"].numpy(), np.asarray(teams[t]["target"], dtype=np.float32).astype(np.float64)), "the target network was written"
        # (float32 values, widened: what the next call takes back as its state; params32: the bits)
        out[t] = dict(params=g["params"].numpy(), exp_avg=g["exp_avg"].numpy(), exp_avg_sq=g["exp_avg_sq"].numpy(), step=float(g["step"]),
                      params32=g["params"].view.cpu().numpy())
    return out


def _workspace(nbytes):
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    ws[nbytes:] = 0x5A
    assert ws.data_ptr() % 256 == 0
    return ws


def abi_step(pkg, env, teams, batch, gamma):
    """One susnet_mlp_train_step by hand.  teams: per team None or dict(dims, params, target, lr, betas[, eps, exp_avg, exp_avg_sq,
    step]); batch: dict of numpy arrays feat, next_feat [n][F], idx [n], actions [M][A], rewards [M][A], dones [M], imposters [M].
    -> (losses [2], per team dict of float64 numpy params / exp_avg / exp_avg_sq / step)."""
    L = pkg._lib
    io = L.MlpTrainIO()
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
    n = len(batch["idx"])
    feat, next_feat = dev(batch["feat"], torch.float32), dev(batch["next_feat"], torch.float32)
    idx = dev(batch["idx"], torch.int64)
    actions, rewards = dev(batch["actions"], torch.int64), dev(batch["rewards"], torch.float32)
    dones, imposters = dev(batch["dones"], torch.uint8), dev(batch["imposters"].reshape(-1, 1), torch.int16)
    io.feat, io.next_feat, io.indices, io.n = feat.data_ptr(), next_feat.data_ptr(), idx.data_ptr(), n
    io.actions, io.rewards, io.dones, io.imposters = actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(), imposters.data_ptr()
    io.max_size, io.gamma = actions.shape[0], gamma
    bufs = [None if tm is None else _team_buffers(io.team[t], tm) for t, tm in enumerate(teams)]
    losses = torch.full((4,), CANARY, dtype=torch.float32, device=DEV)  # [canary, imposter, crew, canary]
    io.losses_out = losses.data_ptr() + 4
    nbytes = C.c_uint64()
    L.check(env.lib.susnet_mlp_train_workspace_bytes(env._h, C.byref(io), C.byref(nbytes)))
    ws = _workspace(int(nbytes.value))
    io.workspace, io.workspace_bytes = ws.data_ptr(), int(nbytes.value)
    with torch.cuda.device(DEV):
        L.check(env.lib.susnet_mlp_train_step(env._h, C.byref(io), env._stream()))
    torch.cuda.synchronize()
    lo = losses.cpu().numpy()
    assert lo[0] == CANARY and lo[3] == CANARY, "losses_out: a neighbour was written"
    assert bool((ws[int(nbytes.value):] == 0x5A).all()), "the workspace was overrun"
    return lo[1:3].astype(np.float64), _team_results(bufs, teams)


def fused_abi_step(pkg, env, layout, teams, case, gamma, packed=False):
    """One susnet_dqn_train_step by hand on the case's ring (fused_case / float_case).  teams: as abi_step's.  Canaries stand in front of
    and behind everything the call writes -- params, exp_avg, exp_avg_sq (an ODD 4-byte offset: include/susnet.h asks for nothing
    beyond a float's alignment), losses_out, the packed images (16-byte aligned, handed in full of NaN) and the workspace past
    susnet_dqn_workspace_bytes (256-byte aligned) -- and the target buffer must come back unchanged.  packed: hand in an image per
    team to rewrite.  -> (losses [2], per team dict of float64 params / exp_avg / exp_avg_sq / step and `image`, the float32 image or
    None)."""
    L = pkg._lib
    lay = X.LAYOUTS[layout]
    batch, ring = case["batch"], case["ring"]
    io = L.DqnIO()
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
    comps = lay["comps"]
    io.n_components, io.trajectory_size = len(comps), 1
    for i, c in enumerate(comps):
        io.components[i] = L.FLAT_COMPONENTS[c]
    assert env.n_agents == lay["A"] and env.flattened_state_size == ring["states"].shape[1]
    states, next_states = dev(ring["states"], torch.float32), dev(ring["next_states"], torch.float32)
    idx = dev(batch["idx"], torch.int64)
    actions, rewards = dev(batch["actions"], torch.int64), dev(batch["rewards"], torch.float32)
    dones, imposters = dev(batch["dones"], torch.uint8), dev(batch["imposters"].reshape(-1, 1), torch.int16)
    assert states.shape[0] == actions.shape[0] == rewards.shape[0] == dones.shape[0] == imposters.shape[0]
    io.states, io.next_states, io.indices, io.n = states.data_ptr(), next_states.data_ptr(), idx.data_ptr(), len(batch["idx"])
    io.actions, io.rewards, io.dones, io.imposters = actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(), imposters.data_ptr()
    io.max_size, io.gamma = actions.shape[0], gamma
    bufs, images = [None, None], [None, None]
    n_image = X.image_offsets(layout)["packed"]
    for t, tm in enumerate(teams):
        if tm is None:
            continue
        bufs[t] = _team_buffers(io.team[t], tm)
        if packed:
            images[t] = Guarded(n=n_image, lead=4, fill=float("nan"))
            io.team[t].packed = images[t].ptr()
    losses = torch.full((4,), CANARY, dtype=torch.float32, device=DEV)  # [canary, imposter, crew, canary]
    io.losses_out = losses.data_ptr() + 4
    nbytes = C.c_uint64()
    L.check(env.lib.susnet_dqn_workspace_bytes(env._h, C.byref(io), C.byref(nbytes)))
    ws = _workspace(int(nbytes.value))
    io.workspace, io.workspace_bytes = ws.data_ptr(), int(nbytes.value)
    with torch.cuda.device(DEV):
        L.check(env.lib.susnet_dqn_train_step(env._h, C.byref(io), env._stream()))
    torch.cuda.synchronize()
    lo = losses.cpu().numpy()
    assert lo[0] == CANARY and lo[3] == CANARY, "losses_out: a neighbour was written"
    assert bool((ws[int(nbytes.value):] == 0x5A).all()), "the workspace was overrun"
    out = _team_results(bufs, teams)
    for t, im in enumerate(images):
        if out[t] is not None:
            out[t]["image"] = None
        if im is not None:
            assert im.intact(), f"team {t} packed image: a canary was overwritten"
            out[t]["image"] = im.view.cpu().numpy()
    return lo[1:3].astype(np.float64), out


def same_bits(a, b):
    """float32 arrays equal bit for bit (the sign of a zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the exact cases of the fused step (test_train_exact_host.py states their properties on the reference, test_gpu_train_exact.py runs them)
STACKS = ("reference", "caps", "ragged", "padded", "ones")


def stack_dims(layout, stack):
    """(imposter stack, crew stack) of a named stack: `reference` [F, 256, 128, 64, 16, n_act] (the reference's MLP), `caps` (every width
    at its cap: 67 weight-gradient tiles, 512 bias threads), `ragged` (one past and one short of a 32-block), `padded`, `ones`."""
    lay = X.LAYOUTS[layout]
    F, acts = lay["F"], (lay["n_imp"], lay["n_crew"])
    return {"reference": [[F, 256, 128, 64, 16, n] for n in acts], "caps": [[F, 256, 128, 64, 32, 32]] * 2,
            "ragged": [[F, 33, 31, 17, 5, n] for n in acts], "padded": [[F, 200, 100, 50, 10, 5]] * 2, "ones": [[F, 1, 1, 1, 1, 1]] * 2}[stack]


def _counts(layout, *c):
    return tuple(c) + (0,) * (X.LAYOUTS[layout]["A"] - len(c))


# (layout, stack, n, counts): one tile per workgroup.  n = 64 split between agents 0 and 1 (on onehot3 agent 2's imposter update is empty and
# its crew list is the whole batch); n = 64 with agent 0 always the imposter (the production 1v1 case); n = 128: G = 4 workgroups, lists of
# 64 rows -- two workgroups get no tile and write zero partials
ONE_TILE_CASES = [(layout, stack, n, _counts(layout, *c)) for layout in ("onehot1", "onehot3", "coord1") for stack in STACKS
                  for n, c in ((64, (32, 32)), (64, (64, 0)), (128, (64, 64)))]
# n = 16384: G = 256 workgroups; a list of 16384 rows is 512 tiles, two per workgroup through the register accumulators
TWO_TILE_CASES = [("onehot1", "ragged", 16384, (16384, 0)), ("onehot3", "ragged", 16384, (8192, 8192, 0)), ("onehot3", "reference", 16384, (8192, 8192, 0))]
# seeds other than 0, found by trying 0, 1, 2, .. on the CPU until the REFERENCE meets test_train_exact_host.py's coverage conditions
CASE_SEEDS = {("onehot1", "ones", 64, (32, 32)): 7, ("onehot1", "ones", 64, (64, 0)): 108, ("onehot1", "ones", 128, (64, 64)): 19,
              ("onehot3", "ones", 64, (32, 32, 0)): 24, ("onehot3", "ones", 64, (64, 0, 0)): 24, ("onehot3", "ones", 128, (64, 64, 0)): 1}


def case_id(case_key):
    layout, stack, n, counts = case_key
    return f"{layout}-{stack}-{n}-{'+'.join(map(str, counts))}"


def one_tile_case(case_key):
    """slope 0.5, gamma 0.5; 4 nonzero weights per unit on the one-hot layouts, 2 on coord1 (its coordinates up to 8 multiply through:
    with 4 the worst sum passes 2^24)."""
    layout, stack, n, counts = case_key
    return fused_case(layout, stack_dims(layout, stack), n, counts, CASE_SEEDS.get(case_key, 0), slope=0.5, gamma=0.5, nnz=2 if layout == "coord1" else 4)


def two_tile_case(case_key):
    """slope 1, gamma 1, 2 nonzero weights per unit: at 16384 rows slope 0.5 leaves no layout exact.  With slope 1 the forward no
    longer depends on the sign of z; the slope gradient (the sum of z dh over z <= 0) still does."""
    layout, stack, n, counts = case_key
    case = fused_case(layout, stack_dims(layout, stack), n, counts, CASE_SEEDS.get(case_key, 0), slope=1.0, gamma=1.0, nnz=2)
    if stack == "reference":  # the crew team alone (it owns the 16384-row list): the restatement of both teams takes too long for one test
        case["enabled"] = (False, True)
    return case


# ---- the Adam case: the one k_train_adam, reached from both train steps, on one exact batch -------------------------------------------------
ADAM_CASE = ("onehot1", "reference", 64, (64, 0))  # agent 0 the imposter on every row: each team has ONE non-empty update per call
ADAM_BETAS = (0.5, 0.75)
ADAM_LRS = (0.0, 0.0, 0.0, 2.0 ** -6)  # the learning rate of calls 1 .. 4
U32 = 2.0 ** -24  # float32's unit roundoff (round to nearest)


def adam_eps(grad):
    """A power of two at the median magnitude of the non-zero gradient entries.  The gradient is the same in every call (lr = 0 until
    the last), so sqrt(v) / sqrt(bc2) = |g| at every step: eps and the root are of one size over the bulk of the entries, and a
    misplaced eps moves the update by a large factor."""
    nz = np.abs(grad[grad != 0])
    return float(2.0 ** round(float(np.median(np.log2(nz)))))


def adam_eps_share(grad, eps):
    """The share of the non-zero-gradient entries with eps within 1/16 .. 16 times sqrt(v) / sqrt(bc2) (= |g|)."""
    nz = np.abs(grad[grad != 0])
    return float(((eps >= nz / 16) & (eps <= nz * 16)).mean())


def adam_bounds(g, p, update):
    """Per element, the most the float32 kernel may differ from float64 Adam after up to 4 steps on a constant, float32-exact gradient g
    with betas (0.5, 0.75), counted from tr_adam's operations (u = 2^-24; every float32 operation is off by at most u of its result,
    sqrtf and the divisions are allowed 2 u):
      m = m + 0.5 (g - m): 2 roundings a step (the difference, the sum; the product with 0.5 is exact), each at most u |g| since |m| and
        |g - m| stay below |g|: at most 1.5 u |g| fresh, and the carried error halves every step: 3 u |g|.  Bound: 4 u |g|.
      v = 0.75 v + 0.25 g g: 3 roundings (g g, 0.75 v, the sum; the product with 0.25 is exact), at most (0.25 + 0.75 + 1) u g^2 fresh,
        the carried error shrinks by 0.75: 8 u g^2.  Bound: 9 u g^2.
      update = (float)(lr / bc1) (m / (sqrtf(v) / (float)sqrt(bc2) + eps)) at step 4, relative: m 4 / 0.9375 = 4.3 u; v 9 / 0.684 =
        13.2 u, halved by the root = 6.6 u; sqrtf 2 u, (float)sqrt(bc2) u, the division 2 u, + eps u (eps itself is exact), the
        conversion of lr / bc1 u, m / denom 2 u, the product u: 20.9 u, c1 = 24.  The final add rounds once more: u (|p| + |update|).
    -> (|m - m64|, |v - v64|, |p - p64|) bounds; zero where g = 0 (m = v = 0 and p unchanged, bit for bit)."""
    g, p, update = (np.abs(np.asarray(x, dtype=np.float64)) for x in (g, p, update))
    return 4 * U32 * g, 9 * U32 * g * g, np.where(g == 0, 0.0, 25 * U32 * update + U32 * p)
