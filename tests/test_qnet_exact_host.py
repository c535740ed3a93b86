"""CPU checks behind the exact tests of the fused Q-network kernels (tests/qnet_exact.py): the integer networks are exact in float32 on
the directed states, the states and tie networks cover what test_gpu_qnet_exact.py relies on -- conditions on the INPUTS, met by the
float64 reference alone -- and the host packer (susnet_qnet_pack), evaluated through a numpy restatement of how the kernels read its
image, reproduces the float64 reference exactly on all three compiled-in layouts.  No kernel is launched here."""
import importlib

import numpy as np
import pytest

import qnet_exact as X


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_directed_states_cover_the_layer_one_image(layout):
    lay = X.LAYOUTS[layout]
    A, N = lay["A"], lay["N"]
    st, rows = X.directed_states(layout), X.oracle_rows(layout)
    assert len(rows) == X.N_STATES and int(st["playable"].sum()) == X.N_STATES - X.N_SPECIAL
    assert st["pos"].min() == 0 and st["pos"].max() == N - 1
    if lay["dead_zero"]:  # every feature column is set in some row: every position row of the image is gathered
        assert (rows != 0).any(axis=0).all(), np.flatnonzero(~(rows != 0).any(axis=0))
    else:  # every coordinate value per coordinate, and a dead agent whose non-zero coordinates stay in the row
        for c in range(lay["F"]):
            assert set(rows[:, c].astype(int)) == set(range(N)), c
        dead = st["alive"] == 0
        assert (dead & (st["pos"] > 0).all(axis=2)).any(axis=0).all()
        assert np.array_equal(rows, st["pos"].reshape(len(rows), 2 * A).astype(np.float32))
    # every alive combination; the imposter dead; the imposter at each index where the game shuffles it
    assert {tuple(a) for a in st["alive"].tolist()} == {tuple((b >> i) & 1 for i in range(A)) for b in range(2 ** A)}
    assert ((st["alive"] == 0) & (st["imp"] == 1)).any()
    assert set(st["imp"].argmax(axis=1).tolist()) == (set(range(A)) if lay["shuffle"] else {0}) and (st["imp"].sum(axis=1) == 1).all()
    # the tail bits as the kernel builds them are the oracle row's, and every reachable value occurs: alive bits x the one-hot closest bit
    tails = [X.tail_value(layout, st["pos"][k], st["alive"][k]) for k in range(len(rows))]
    if lay["tail_bits"]:
        one_hot = A * 2 * N
        from_rows = (rows[:, one_hot:].astype(int) << np.arange(lay["tail_bits"])).sum(axis=1)
        assert np.array_equal(np.array(tails), from_rows)
        # alive (crew 1, crew 2) | closest: both dead -> first; one dead -> the other (an alive one is nearer than 2 N); both alive -> either
        assert set(tails) == {0b0100, 0b0101, 0b1010, 0b0111, 0b1011}
        both = (st["alive"][:, 1] == 1) & (st["alive"][:, 2] == 1)
        d = np.abs(st["pos"][:, :1] - st["pos"][:, 1:]).sum(axis=2)
        assert (both & (d[:, 0] == d[:, 1]) & (d[:, 0] > 0)).any(), "equal distances: the first minimum"
    else:
        assert set(tails) == {0}
    # playable: what a step may follow
    free = X.grid_of(layout)
    for k in np.flatnonzero(st["playable"]):
        assert all(free[x, y] for x, y in st["pos"][k]) and (st["alive"][k][st["imp"][k] == 1] == 1).all() and (st["alive"][k][st["imp"][k] == 0] == 1).any()
    assert not free[st["pos"][~st["playable"]][..., 0], st["pos"][~st["playable"]][..., 1]].all(), "somebody stands on a wall cell"
    # every batch of the forward test beyond B = 1 holds states that are not playable
    assert (~st["playable"][:31]).sum() >= 4


@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_integer_networks_are_exact_on_the_directed_rows(layout):
    """Every (stack, slope set) case: reference_q asserts the exactness condition; the worst bound stays far below 2^24."""
    rows = X.oracle_rows(layout)
    worst = 0.0
    for si in range(len(X.SLOPE_SETS)):
        cases = X.forward_cases(layout, si)
        assert len(cases) == 2 + 2 * len(X.N_OUT)
        for dims, net in cases:
            q, share = X.reference_q(net, rows)
            assert q.shape == (len(rows), dims[-1])
            worst = max(worst, share)
    print(f"{layout}: {len(rows)} directed states, worst exactness bound {100 * worst:.2f} % of 2^24")
    assert worst <= 0.25


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_tie_networks_decide_the_argmax_by_ties(layout, which):
    """On the playable states in the order the tick test imports them: every tie group is the row maximum in an environment of either
    32-environment tile of a wave, at least 25 % of the rows have a tied maximum (net B: at least 10 % an untied one), and the kernel's
    two-half argmax rule, restated, gives numpy's first maximum -- with rows in which the halves' maxima are EQUAL, so that the
    `pv == hv && pn < hn` branch is what decides."""
    lay = X.LAYOUTS[layout]
    rows = X.playable_rows(layout)
    assert len(rows) == X.TICK_BATCH
    for n_act in (lay["n_imp"], lay["n_crew"]):
        groups = X.TIE_GROUPS[which][n_act]
        net = X.tie_network(layout, which, n_act)
        q, _ = X.reference_q(net, rows)
        for g in groups:
            assert (q[:, list(g)] == q[:, [g[0]]]).all(), "the group's entries are identical in every environment"
        hit, tied, untied = X.tie_coverage(q, groups)
        print(f"{layout} net {which} {n_act} actions: tied maximum {100 * tied:.1f} %, untied {100 * untied:.1f} %")
        assert all(lo and hi for lo, hi in hit.values()), hit
        assert tied >= 0.25 and (which == "A" or untied >= 0.10), (tied, untied)
        best, cross = X.kernel_argmax(q)
        assert np.array_equal(best, q.argmax(axis=1))
        assert cross.any(), "no row whose two lane halves hold the same maximum"


@pytest.mark.parametrize("layout", sorted(X.LAYOUTS))
def test_packed_image_read_like_the_kernel_equals_the_float64_reference(pkg, layout):
    """susnet_qnet_pack through the image: tail rows by value, the zero row, the k x W1 rows of the coordinate layout, the MFMA-step
    order of the weight stream and the zero padding, on every directed state, for every stack and slope set and the tie networks."""
    L = pkg._lib
    lay = X.LAYOUTS[layout]
    st, rows = X.directed_states(layout), X.oracle_rows(layout)
    h = X.host_handle(L, layout)
    try:
        nets = [net for si in range(len(X.SLOPE_SETS)) for _, net in X.forward_cases(layout, si)]
        nets += [X.tie_network(layout, which, n) for which in "AB" for n in (lay["n_imp"], lay["n_crew"])]
        for net in nets:
            image = X.host_pack(L, h, layout, net)
            assert not np.isnan(image).any(), "the packer writes the whole image"
            n_out = net[0][4].shape[0]
            want, _ = X.reference_q(net, rows)
            X.assert_same_values(X.image_forward(layout, image, st, n_out), want, (layout, [w.shape[0] for w in net[0]], net[2]))
            o = X.image_offsets(layout)
            assert not image[o["zero"] * X.ROW_STRIDE:(o["zero"] + 1) * X.ROW_STRIDE].any(), "the zero row"
    finally:
        L.lib().susnet_destroy(h)
