"""Shared by the exact tests of the fused Q-network kernels (susnet_qnet_forward / susnet_qnet_policy_step): integer-valued networks whose
float64 evaluation every float32 summation order reproduces, directed states for the three compiled-in feature layouts with their feature
rows from the CPU oracle, tie networks for the in-register argmax, and a numpy restatement of how the kernels read a packed image
(susnet_qnet.h).  Used by the CPU test of the host packer (test_qnet_exact_host.py) and the GPU test (test_gpu_qnet_exact.py); nothing
here touches a GPU, and the package / the oracle are handed in or imported inside the functions that need them."""
import ctypes as C
import functools

import numpy as np

# ---- the three compiled-in layouts ------------------------------------------------------------------------------------------------------
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]
ITG_KW = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
LAYOUTS = {
    # F: input width; A, N: agents, grid size; tail_bits: bits behind the position one-hots; dead_zero: a dead agent's positions read the zero row
    "onehot1": dict(game="itg", comps=["onehot_pos"], F=36, A=2, N=9, tail_bits=0, dead_zero=True, n_imp=6, n_crew=5, shuffle=False),
    "coord1": dict(game="itg", comps=["coord_pos"], F=4, A=2, N=9, tail_bits=0, dead_zero=False, n_imp=6, n_crew=5, shuffle=False),
    "onehot3": dict(game="base", comps=COMPS3, F=88, A=3, N=14, tail_bits=4, dead_zero=True, n_imp=7, n_crew=6, shuffle=True),
}
N_OUT = (1, 4, 5, 8, 9, 31, 32)  # brackets the lane-half boundaries (output row n lives in half (n / 4) % 2) and the padded width
BATCHES = (1, 31, 33, 64, 65, 257, 300)  # the tile of 32, the wave of 64, the workgroup of 256
TICK_BATCH = 257  # the one-kernel tick's batch: a ragged last wave
N_STATES, N_SPECIAL = 300, 40
SLOPE_SETS = (
    (0.5, 0.25, 1.0, 0.5),    # every slope in [0, 1]: the max(x, s x) form
    (1.0, 0.0, 0.5, 0.25),    # ... at both ends of that interval
    (0.5, -0.5, -1.0, 0.25),  # slopes outside it: compare / select
)


def grid_of(layout):
    """``grid[x, y]`` True = free: the four-room map of the layout's game (9x9: the reference's walls; 14x14: sus-net_amd.four_room_grid)."""
    n = LAYOUTS[layout]["N"]
    g = np.ones((n, n), dtype=bool)
    if n == 9:
        for i, j in [(0, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (8, 4), (4, 0), (4, 2), (4, 3), (4, 5), (4, 6), (4, 8)]:
            g[i, j] = False
        return g
    wall = (n - 1) // 2
    doors = ((wall - 1) // 2, wall + 1 + (n - 1 - wall) // 2)
    for i in range(n):
        if i not in doors:
            g[i, wall] = g[wall, i] = False
    return g


def stacks(layout):
    """The layer stacks of the forward test: nothing padded, padded widths, one past / one short of a 32-block, the narrowest."""
    F = LAYOUTS[layout]["F"]
    out = [[F, 256, 128, 64, 32, 32]]
    out += [[F, 200, 100, 50, 10, n] for n in N_OUT]
    out += [[F, 33, 31, 17, 5, n] for n in N_OUT]
    out += [[F, 1, 1, 1, 1, 1]]
    return out


# ---- integer networks and their float64 evaluation --------------------------------------------------------------------------------------
def int_network(dims, seed, slopes, p_zero=0.4):
    """``(W, b, slopes)``: five Linear layers ``W[l] [dims[l + 1], dims[l]]`` / ``b[l]`` with entries from {-1, 0, 1} (``p_zero``: the
    share of zero weights) and four dyadic PReLU slopes."""
    assert len(dims) == 6 and len(slopes) == 4
    rng = np.random.default_rng(seed)
    p = [(1.0 - p_zero) / 2, p_zero, (1.0 - p_zero) / 2]
    W = [rng.choice([-1.0, 0.0, 1.0], size=(dims[l + 1], dims[l]), p=p) for l in range(5)]
    b = [rng.choice([-1.0, 0.0, 1.0], size=dims[l + 1]) for l in range(5)]
    return W, b, tuple(float(s) for s in slopes)


def binary_places(s):
    """Binary places behind the point of a dyadic slope: how many a PReLU of that slope adds to its input's."""
    for p in range(8):
        if float(s) * 2.0 ** p == np.floor(float(s) * 2.0 ** p):
            return p
    raise AssertionError(f"slope {s} is not dyadic")


def reference_q(net, rows):
    """The network in float64 on feature rows ``[n, F]``: z = h W^T + b, PReLU as z > 0 ? z : s z, no activation after the last layer.
    Returns ``(q float32 [n, n_out], share)``; ``share`` = the worst layer's bound as a fraction of 2^24.

    Asserted, because it is what makes float32 exact in ANY summation order: with P binary places behind the point accumulated by the
    slopes passed so far, every input, product and partial sum of a layer is a multiple of 2^-P of magnitude at most
    max(sum |w||h| + |b|), so it is a float32 value if that bound times 2^P is at most 2^24 (the same for an activation's output with the
    places its slope adds); and the float64 result round-trips through float32."""
    W, b, slopes = net
    h = np.asarray(rows, dtype=np.float64)
    assert np.array_equal(h, np.floor(h)), "feature rows are integers"
    places, share = 0, 0.0
    for l in range(5):
        bound = float((np.abs(h) @ np.abs(W[l]).T + np.abs(b[l])).max()) * 2.0 ** places
        assert bound <= 2.0 ** 24, (l, bound)
        share = max(share, bound / 2.0 ** 24)
        z = h @ W[l].T + b[l]
        if l < 4:
            h = np.where(z > 0, z, slopes[l] * z)
            places += binary_places(slopes[l])
            assert float(np.abs(h).max()) * 2.0 ** places <= 2.0 ** 24, (l, "activation")
        else:
            h = z
    q = h.astype(np.float32)
    assert np.array_equal(q.astype(np.float64), h) and not np.isnan(q).any()
    return q, share


def assert_same_values(got, want, what=""):
    """Equal by VALUE and NaN-free: a slope of 0 yields -0.0 where another order of the same exact operations yields +0.0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    assert not np.isnan(got).any(), (what, "NaN")
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def net_seed(layout, stack_index, slope_index):
    return 1000 * (1 + sorted(LAYOUTS).index(layout)) + 10 * stack_index + slope_index


def forward_cases(layout, slope_index):
    """``(dims, net)`` for every stack of the layout under one slope set."""
    return [(dims, int_network(dims, net_seed(layout, k, slope_index), SLOPE_SETS[slope_index])) for k, dims in enumerate(stacks(layout))]


# ---- tie networks ------------------------------------------------------------------------------------------------------------------------
# groups of output indices whose Q entries are identical in every environment; {3, 4} and {1, 4, 5} straddle the two lane halves
TIE_GROUPS = {
    "A": {7: [(0, 1), (3, 4), (2, 5, 6)], 6: [(0, 1), (3, 4), (2, 5)], 5: [(0, 1), (3, 4)]},  # every index tied but index 2 of five
    "B": {7: [(1, 4, 5), (2, 6)], 6: [(1, 4, 5)], 5: [(2, 4), (0, 3)]},                      # free indices: untied maxima occur too
}
TIE_SLOPES = {"A": 0, "B": 2}  # net A on the max(x, s x) form, net B on compare / select
# chosen so that the REFERENCE satisfies the coverage conditions test_qnet_exact_host.py states (every group the row maximum in both lane
# halves, the tied / untied shares): a property of the inputs, found by trying seeds 0, 1, 2, .. on the CPU
TIE_SEEDS = {("onehot1", "A", 6): 0, ("onehot1", "A", 5): 0, ("onehot1", "B", 6): 0, ("onehot1", "B", 5): 1,
             ("coord1", "A", 6): 0, ("coord1", "A", 5): 0, ("coord1", "B", 6): 13, ("coord1", "B", 5): 9,
             ("onehot3", "A", 7): 0, ("onehot3", "A", 6): 1, ("onehot3", "B", 7): 2, ("onehot3", "B", 6): 4}


def tie_network(layout, which, n_act, seed=None):
    """An integer network ``[F, 200, 100, 50, 10, n_act]`` whose last layer repeats, per group of TIE_GROUPS, the first member's row of W5
    and bias entry on the other members."""
    lay = LAYOUTS[layout]
    seed = TIE_SEEDS[(layout, which, n_act)] if seed is None else seed
    W, b, slopes = int_network([lay["F"], 200, 100, 50, 10, n_act], 50_000 + seed, SLOPE_SETS[TIE_SLOPES[which]])
    for group in TIE_GROUPS[which][n_act]:
        for n in group[1:]:
            W[4][n] = W[4][group[0]]
            b[4][n] = b[4][group[0]]
    return W, b, slopes


def tie_coverage(q, groups):
    """Of Q rows in the order the GPU test imports their states: per group whether it is the row maximum in some environment of the first
    and of the second 32-environment tile of a wave; the shares of rows whose maximum is attained more than once / exactly once."""
    top = q.max(axis=1)
    n_top = (q == top[:, None]).sum(axis=1)
    low = (np.arange(len(q)) % 64) < 32
    hit = {g: (bool((q[low, g[0]] == top[low]).any()), bool((q[~low, g[0]] == top[~low]).any())) for g in groups}
    return hit, float((n_top > 1).mean()), float((n_top == 1).mean())


def kernel_argmax(q):
    """The greedy action as qnet_wave takes it: each lane half walks ITS entries of the row (row n lives in half (n / 4) % 2) in ascending
    n keeping the first maximum, then the halves are compared -- the other half's wins if it is larger, or equal with the smaller index.
    Returns ``(argmax [n], decided_by_tie [n])``: the second marks rows where the two halves' maxima were equal."""
    n, n_out = q.shape
    best = np.zeros(n, dtype=np.int64)
    tied = np.zeros(n, dtype=bool)
    for b in range(n):
        half = []
        for h in (0, 1):
            hv, hn = -np.inf, None
            for k in range(n_out):
                if (k // 4) % 2 == h and (hn is None or q[b, k] > hv):
                    hv, hn = q[b, k], k
            half.append((hv, hn))
        (hv, hn), (pv, pn) = half
        theirs = pn is not None and (hn is None or pv > hv or (pv == hv and pn < hn))
        tied[b] = pn is not None and hn is not None and pv == hv
        best[b] = pn if theirs else hn
    return best, tied


# ---- directed states ---------------------------------------------------------------------------------------------------------------------
def _free_cell(rng, free):
    xs, ys = np.nonzero(free)
    k = int(rng.integers(len(xs)))
    return int(xs[k]), int(ys[k])


def _is_playable(lay, free, pos, alive, imp):
    """A state a step may follow: the imposter alive, at least one crew member alive, nobody on a wall cell."""
    crew_alive = any(alive[i] and not imp[i] for i in range(lay["A"]))
    imp_alive = all(alive[i] for i in range(lay["A"]) if imp[i])
    return bool(imp_alive and crew_alive and all(free[x, y] for x, y in pos))


@functools.lru_cache(maxsize=None)
def directed_states(layout):
    """``pos [n, A, 2]``, ``alive [n, A]``, ``imp [n, A]`` (the imposter mask), ``playable [n]``, n = N_STATES, read-only.  They cover:
    every coordinate value of x and of y for every agent (alive: every position row of the layer-1 image is gathered); every alive
    combination, a dead imposter and (1v2) both crew dead included; dead agents at non-zero coordinates (the coordinate layout does not
    zero them); on 1v2 crew 1 nearer, crew 2 nearer, equal distances, either crew dead, and the imposter at each agent index; agents on
    wall cells and in the corners.  N_SPECIAL of them are not playable (index % 7 == 3: every batch of the forward test but B = 1 holds
    some); the tick tests import the playable ones."""
    lay = LAYOUTS[layout]
    A, N = lay["A"], lay["N"]
    free = grid_of(layout)
    rng = np.random.default_rng(77 + N)
    walls = np.argwhere(~free)
    play, special = [], []

    def imp_at(m):
        return [int(i == m) for i in range(A)]

    def add(pos, alive, imp):
        st = (np.array(pos, dtype=np.int64).reshape(A, 2), np.array(alive, dtype=np.uint8), np.array(imp, dtype=np.uint8))
        (play if _is_playable(lay, free, *st) else special).append(st)

    def random_imp():
        return imp_at(int(rng.integers(A)) if lay["shuffle"] else 0)

    # every coordinate value, all agents alive, on free cells: state (c, k) puts coordinate c of agent i at (k + 3 i) % N
    for c in (0, 1):
        for k in range(N):
            pos = []
            for i in range(A):
                v = (k + 3 * i) % N
                other = rng.permutation(N)
                o = next(int(o) for o in other if (free[v, o] if c == 0 else free[o, v]))
                pos.append((v, o) if c == 0 else (o, v))
            add(pos, [1] * A, imp_at(k % A if lay["shuffle"] else 0))
    if A == 3:  # the closest-crew bit: agent 0 against agents 1 and 2, for the imposter at every index
        for m in range(A):
            for want in ("first", "second", "equal", "first dead", "second dead"):
                while True:
                    pos = [_free_cell(rng, free) for _ in range(A)]
                    d1 = abs(pos[0][0] - pos[1][0]) + abs(pos[0][1] - pos[1][1])
                    d2 = abs(pos[0][0] - pos[2][0]) + abs(pos[0][1] - pos[2][1])
                    alive = [1, int(want != "first dead"), int(want != "second dead")]
                    ok = {"first": d1 < d2, "second": d2 < d1, "equal": d1 == d2 and d1 > 0, "first dead": d1 < d2, "second dead": d2 < d1}[want]
                    if ok:  # (the imposter itself dead: not playable -- add() files it with the others of that kind)
                        break
                add(pos, alive, imp_at(m))
    # not playable: every alive combination with somebody dead who must not be (at random cells, non-zero coordinates among them), ...
    for m in (range(A) if lay["shuffle"] else (0,)):
        for bits in range(2 ** A):
            alive = [(bits >> i) & 1 for i in range(A)]
            pos = [_free_cell(rng, free) for _ in range(A)]
            if not _is_playable(lay, free, pos, alive, imp_at(m)):
                add(pos, alive, imp_at(m))
    # ... the corners with somebody dead, and agents on wall cells (alive and dead)
    corners = [(0, 0), (N - 1, N - 1), (0, N - 1), (N - 1, 0)]
    for k in range(4):
        add([corners[(k + i) % 4] for i in range(A)], [int(i != k % A) for i in range(A)] if A == 2 else [int(i == k % A) for i in range(A)], imp_at(0))
    for k in range(6):
        pos = [_free_cell(rng, free) for _ in range(A)]
        pos[k % A] = tuple(int(v) for v in walls[int(rng.integers(len(walls)))])
        add(pos, [1] * A if k < 3 else [int(i != k % A) for i in range(A)], random_imp())
    while len(special) < N_SPECIAL:  # the rest: random states that are not playable
        pos = [tuple(int(v) for v in rng.integers(0, N, size=2)) for _ in range(A)]
        alive = [int(v) for v in rng.integers(0, 2, size=A)]
        imp = random_imp()
        if not _is_playable(lay, free, pos, alive, imp):
            add(pos, alive, imp)
    assert len(special) == N_SPECIAL, len(special)
    while len(play) < N_STATES - N_SPECIAL:  # the rest: random playable states
        pos = [_free_cell(rng, free) for _ in range(A)]
        alive = [int(v) for v in rng.integers(0, 2, size=A)] if A == 3 else [1, 1]
        imp = random_imp()
        if _is_playable(lay, free, pos, alive, imp):
            add(pos, alive, imp)
    assert len(play) == N_STATES - N_SPECIAL, len(play)
    order, play_it, special_it = [], iter(play), iter(special)
    for i in range(N_STATES):
        order.append(next(special_it) if i % 7 == 3 and i < 7 * N_SPECIAL else next(play_it))
    out = dict(pos=np.stack([s[0] for s in order]), alive=np.stack([s[1] for s in order]), imp=np.stack([s[2] for s in order]))
    out["playable"] = np.array([_is_playable(lay, free, *s) for s in order])
    assert int(out["playable"].sum()) == N_STATES - N_SPECIAL >= TICK_BATCH
    for v in out.values():
        v.setflags(write=False)
    return out


def playable_states(layout):
    """The first TICK_BATCH playable states, in the order the tick tests import them."""
    st = directed_states(layout)
    keep = np.flatnonzero(st["playable"])[:TICK_BATCH]
    return {k: v[keep] for k, v in st.items()}


def oracle_batch(layout, n):
    """The CPU oracle's game of the layout, ``n`` environments."""
    from oracle import oracle as om

    lay = LAYOUTS[layout]
    grid = grid_of(layout).astype(np.uint8)
    if lay["game"] == "itg":
        cfg = om.make_config("itg", grid=grid, shuffle_imposter_index=False, **ITG_KW)
    else:
        cfg = om.make_config("base", n_imposters=1, n_crew=2, n_jobs=4, grid=grid)
    return om.OracleBatch(cfg, n)


def oracle_rows_of(layout, states):
    """FlatFeaturizer rows of states, from the CPU oracle (``OracleBatch.set_state`` then ``obs_flat``: pinned to the reference's
    featurizers by the feat_* fixtures)."""
    n = len(states["pos"])
    ob = oracle_batch(layout, n)
    for k in range(n):
        ob.set_state(k, pos=states["pos"][k], alive=states["alive"][k], imp_mask=states["imp"][k])
    rows = ob.obs_flat(LAYOUTS[layout]["comps"])
    assert rows.shape == (n, LAYOUTS[layout]["F"]) and rows.dtype == np.float32
    return rows


@functools.lru_cache(maxsize=None)
def oracle_rows(layout):
    """The rows of ``directed_states(layout)``: computed once per process, read-only."""
    rows = oracle_rows_of(layout, directed_states(layout))
    rows.setflags(write=False)
    return rows


def playable_rows(layout):
    return oracle_rows(layout)[np.flatnonzero(directed_states(layout)["playable"])[:TICK_BATCH]]


def make_env(pkg, layout, batch, device="cuda:0", seed=7, **kw):
    """The batched env of the layout's game (the GPU tests)."""
    lay = LAYOUTS[layout]
    if lay["game"] == "itg":
        return pkg.BatchedImposterTrainingGround(**ITG_KW, grid=grid_of(layout), batch=batch, device=device, rng="philox", seed=seed, **kw)
    return pkg.BatchedFourRoomEnv(1, 2, 4, grid=grid_of(layout), batch=batch, device=device, rng="philox", seed=seed, **kw)


def import_states(env, states, n=None):
    """``env.set_state`` of the first ``n`` states (the env must have been reset)."""
    n = env.batch if n is None else n
    assert n <= len(states["pos"])
    env.set_state(agent_positions=np.array(states["pos"][:n]), alive_agents=np.array(states["alive"][:n]), imposter_mask=np.array(states["imp"][:n]))


# ---- the packed image as the kernels read it ---------------------------------------------------------------------------------------------
H = (256, 128, 64, 32, 32)  # the compiled-in widths every stack is padded to
ROW_STRIDE = H[0] + 4


def image_offsets(layout):
    """QNet<ROW>'s constants (susnet_qnet.h), in floats."""
    lay = LAYOUTS[layout]
    one_hot = lay["A"] * 2 * lay["N"]
    o = dict(one_hot=one_hot, zero=one_hot, tail=one_hot + 1, rows=one_hot + 1 + (1 << lay["tail_bits"]))
    o["w1"] = -(-o["rows"] * ROW_STRIDE // 1024) * 1024
    off = o["w1"]
    o["bias"] = []
    for l in range(1, 5):
        o["bias"].append(off)
        off += H[l]
    o["lds"] = off
    o["weights"] = []
    for l in range(1, 5):
        o["weights"].append(off)
        off += H[l - 1] * H[l]
    o["slope"] = off
    o["packed"] = off + 4
    return o


def host_handle(L, layout):
    """A library handle of the layout's game without a GPU (``susnet_create`` only: the packer is host code)."""
    lay = LAYOUTS[layout]
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    d = dict(variant=L.VARIANT_ITG if lay["game"] == "itg" else L.VARIANT_BASE, batch=8, n_imposters=1, n_crew=lay["A"] - 1,
             n_jobs=0 if lay["game"] == "itg" else 4, grid_n=lay["N"], max_time_steps=1000, is_action_order_random=int(lay["game"] != "itg"),
             shuffle_imposter_index=int(lay["shuffle"]), tag_reset_interval=50, rng_mode=L.RNG_PHILOX)
    for k, v in d.items():
        setattr(cfg, k, v)
    free = grid_of(layout)
    for i in range(lay["N"]):
        cfg.grid_rows[i] = sum(1 << j for j in range(lay["N"]) if free[i, j])
    h = C.c_void_p()
    rc = L.lib().susnet_create(C.byref(cfg), C.byref(h))
    assert rc == 0, L.lib().susnet_last_error()
    return h


def host_pack(L, h, layout, net):
    """``susnet_qnet_pack`` of an integer network into a NaN-filled host buffer: the packed image, float32."""
    lib = L.lib()
    W, b, slopes = net
    w32 = [np.ascontiguousarray(w, dtype=np.float32) for w in W]
    b32 = [np.ascontiguousarray(v, dtype=np.float32) for v in b]
    sl = np.asarray(slopes, dtype=np.float32)
    comp_ids = [L.FLAT_COMPONENTS[k] for k in LAYOUTS[layout]["comps"]]
    comps = (C.c_int32 * len(comp_ids))(*comp_ids)
    dims = [w32[0].shape[1]] + [w.shape[0] for w in w32]
    cd = (C.c_int32 * 6)(*dims)
    n = lib.susnet_qnet_packed_floats(h, comps, len(comp_ids), cd, 6)
    assert n == image_offsets(layout)["packed"], (n, image_offsets(layout)["packed"])
    out = np.full(n, np.nan, dtype=np.float32)
    wp = (C.c_void_p * 5)(*[w.ctypes.data for w in w32])
    bp = (C.c_void_p * 5)(*[v.ctypes.data for v in b32])
    assert lib.susnet_qnet_pack(h, comps, len(comp_ids), cd, 6, wp, bp, sl.ctypes.data, out.ctypes.data) == 0, lib.susnet_last_error()
    return out


def tail_value(layout, pos, alive):
    """The bits behind the position one-hots as the kernel builds them from the state (FlatRow::build, susnet_flat.h): alive flags of
    agents 1 .. A - 1, then the one-hot of the crew member closest to agent 0 in L1 distance (a dead one counts 2 N; first minimum)."""
    lay = LAYOUTS[layout]
    A, N = lay["A"], lay["N"]
    if lay["tail_bits"] == 0:
        return 0
    v = 0
    for i in range(1, A):
        v |= int(alive[i]) << (i - 1)
    d = [abs(int(pos[0][0]) - int(pos[i][0])) + abs(int(pos[0][1]) - int(pos[i][1])) if alive[i] else 2 * N for i in range(1, A)]
    return v | 1 << (A - 1 + int(np.argmin(d)))


def image_forward(layout, image, states, n_out):
    """A packed image evaluated the way qnet_wave reads it, in float32 with the kernel's operations:
    h1 = the tail row of the state's tail bits + the 2 A position rows (a dead agent's: the zero row on the one-hot layouts; the
    coordinate layout: row c N + value, dead or alive), PReLU; layers 2..5 from the [kb][nb][q][lane][r] blocks of the weight stream --
    lane l of a block holds row 32 nb + l % 32 and, as four float4 q, the columns 32 kb + 8 q + 4 (l / 32) + r -- with the biases of the
    LDS part as the accumulators' initial values and the slopes from the image's end; every slope in [0, 1]: max(x, s x), else compare /
    select.  ALL padded entries take part: a padded weight, bias or row that is not zero shows.  Returns the first ``n_out`` of the 32
    output rows, float32 ``[n, n_out]``."""
    lay = LAYOUTS[layout]
    A, N = lay["A"], lay["N"]
    o = image_offsets(layout)
    assert image.dtype == np.float32 and image.shape == (o["packed"],)
    w1 = image[:o["rows"] * ROW_STRIDE].reshape(o["rows"], ROW_STRIDE)[:, :H[0]]
    slopes = image[o["slope"]:o["slope"] + 4]
    unit = bool(((slopes >= 0) & (slopes <= 1)).all())

    def prelu(x, s):
        m = (x * s).astype(np.float32)
        return np.fmax(x, m) if unit else np.where(x > 0, x, m)

    n = len(states["pos"])
    h = np.zeros((n, H[0]), dtype=np.float32)
    for k in range(n):
        pos, alive = states["pos"][k], states["alive"][k]
        v = w1[o["tail"] + tail_value(layout, pos, alive)].copy()
        for i in range(A):
            there = bool(alive[i]) or not lay["dead_zero"]
            v = v + w1[i * 2 * N + int(pos[i][0]) if there else o["zero"]]
            v = v + w1[i * 2 * N + N + int(pos[i][1]) if there else o["zero"]]
        h[k] = v
    h = prelu(h, slopes[0])
    for l in range(1, 5):
        KP, NP = H[l - 1], H[l]
        blk = image[o["weights"][l - 1]:o["weights"][l - 1] + KP * NP].reshape(KP // 32, NP // 32, 4, 64, 4)
        kb, nb, q, lane, r = np.meshgrid(*[np.arange(s) for s in blk.shape], indexing="ij")
        full = np.full((NP, KP), np.nan, dtype=np.float32)
        full[32 * nb + lane % 32, 32 * kb + 8 * q + 4 * (lane // 32) + r] = blk
        bias = image[o["bias"][l - 1]:o["bias"][l - 1] + NP]
        z = h.astype(np.float64) @ full.astype(np.float64).T + bias.astype(np.float64)
        z32 = z.astype(np.float32)
        assert np.array_equal(z32.astype(np.float64), z) or np.isnan(z).any(), "the image's sums are float32 values"
        h = prelu(z32, slopes[l]) if l < 4 else z32
    return h[:, :n_out]
