"""FourRoomEnvWithTagging with 9 .. 12 agents, without a GPU: the packed-record layout the byte-parallel family gives these games, the
oracle on the reference fixtures of tests/golden/tagging_wide/ (generate_tagging_wide.py: a directed 12-agent vote script and three CRC
streams), and the committed list of family instantiations."""
import ctypes as C
import glob
import importlib
import os
import re
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from test_capi_abi import make_cfg
from test_oracle_checksums import oracle_crc_stream
from test_oracle_golden import _check_pre, _check_state, apply_injection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_DIR = os.path.join(GOLDEN_DIR, "tagging_wide")
CRC_NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WIDE_DIR, "crc_*.npz")))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.mark.parametrize("n_jobs", [0, 3, 8])
@pytest.mark.parametrize("n_imposters,n_crew", [(1, 8), (2, 9), (3, 9), (1, 11), (3, 7)])
def test_wide_tagging_games_have_a_packed_record(pkg, n_imposters, n_crew, n_jobs):
    """susnet_record_layout of a tagging game with 9 .. 12 agents: the family's planar record, a head of A + 3A + 2A + 1 + 2 bytes behind
    the rewards, the raw observation in four segments, no two fields on one byte (the idiom of test_capi_abi.test_packed_record_layouts)."""
    L = pkg._lib
    lib = L.lib()
    h = C.c_void_p()
    lay, info = L.RecordLayout(), L.Layout()
    assert lib.susnet_create(C.byref(make_cfg(L, variant=L.VARIANT_TAGGING, n_imposters=n_imposters, n_crew=n_crew, n_jobs=n_jobs, tag_reset_interval=5)), C.byref(h)) == 0
    assert lib.susnet_get_layout(h, C.byref(info)) == 0
    assert lib.susnet_record_layout(h, C.byref(lay)) == 0
    lib.susnet_destroy(h)
    A, F = info.n_agents, info.obs_raw_size
    assert A == n_imposters + n_crew and F == 3 * A + 3 * n_jobs + 2 * A + 1
    assert (info.n_actions_crew, info.n_actions_imposter, info.action_space_n) == (6 + A - 1, 7 + A - 1, 8 + A)  # tagging.py:35-60, 68-75
    assert lay.record_bytes > 0 and lay.record_bytes % 4 == 0 and lay.planar == 1
    head = A + 3 * A + 2 * A + 1 + 2
    assert lay.record_bytes == 4 * A + (head + 3) // 4 * 4 + 16 + 8  # rewards | head | eight job-cell slots | eight job-status slots
    assert lay.n_obs_segments == 4
    segs = [tuple(lay.obs_segments[k]) for k in range(4)]
    assert sum(n for _, n in segs) == F and segs[0] == (lay.off_obs, 3 * A) and segs[3] == (8 * A, 2 * A + 1)
    assert (segs[1][1], segs[2][1]) == (2 * n_jobs, n_jobs)
    used = [False] * lay.record_bytes
    for off, n in [(lay.off_rewards, 4 * A), (lay.off_actions, A), (lay.off_done, 1), (lay.off_truncated, 1)] + segs:
        assert 0 <= off and off + n <= lay.record_bytes and not any(used[off:off + n]), (off, n)
        used[off:off + n] = [True] * n


def test_thirteen_agents_still_have_no_packed_record(pkg):
    L = pkg._lib
    lib = L.lib()
    h = C.c_void_p()
    lay = L.RecordLayout()
    for kw in (dict(n_imposters=4, n_crew=9, n_jobs=2), dict(variant=L.VARIANT_TAGGING, n_imposters=3, n_crew=10, n_jobs=2)):
        assert lib.susnet_create(C.byref(make_cfg(L, **kw)), C.byref(h)) == 0
        assert lib.susnet_record_layout(h, C.byref(lay)) == 0
        lib.susnet_destroy(h)
        assert lay.record_bytes == 0, kw


def test_oracle_replays_the_directed_twelve_agent_votes(oracle_mod):
    """test_oracle_golden.test_oracle_replays_reference_trace on tagging_wide/directed_tagging12_votes: state, order, reward bit patterns,
    flags, the 13 counters and the MT19937 words consumed, step by step; and the script reached what it was written for."""
    g = load_golden(os.path.join(WIDE_DIR, "directed_tagging12_votes.npz"))
    meta = g["meta"]
    ob = oracle_mod.OracleBatch(oracle_mod.config_from_fixture_meta(meta), 1)
    assert ob.A == meta["n_agents"] == 12 and ob.J == meta["n_jobs"]
    ob.seed_mt([meta["seed"]])
    ob.reset()
    assert ob.cursor[0] == g["words"][0]
    S = len(g["done"])
    for s in range(S):
        tag = f"directed_tagging12_votes step {s}"
        if g["inject"][s]:
            apply_injection(ob, g, s)
        _check_pre(ob, g, s, tag)
        rew, done, trunc, rc = ob.step_one(0, g["actions"][s])
        assert rc == 0
        np.testing.assert_array_equal(ob.order[0], g["order"][s], err_msg=f"{tag} order")
        _check_state(ob, g, s, tag)
        assert rew.view(np.uint64).tolist() == g["rewards"][s].view(np.uint64).tolist(), f"{tag} rewards {rew} vs {g['rewards'][s]}"
        assert done == bool(g["done"][s]) and trunc == bool(g["trunc"][s]), f"{tag} done/trunc"
        np.testing.assert_array_equal(ob.metrics[0], g["metrics"][s], err_msg=f"{tag} metrics")
        assert ob.cursor[0] == g["words"][s + 1], f"{tag} raw words consumed"
    # what the fixture pins: a count of 11, a vote that ejected an agent of the third word, the 6/6 tie resolved to index 3, a count that
    # survived a same-step kill, an imposter voted out
    assert g["counts"].max() == 11 and g["counts"][0, 11] == 11 and g["alive"][1, 11] == 0
    assert g["counts"][2, 3] == 6 and g["counts"][2, 9] == 6 and g["alive"][3, 3] == 0 and g["alive"][3, 9] == 1
    assert any(g["metrics"][s, 0] > g["metrics"][s - 1, 0] and g["counts"][s].max() >= 4 for s in range(1, S))
    assert g["metrics"][-1, 1] == 3 and g["metrics"][-1, 2] >= 9  # IMP_VOTED_OUT, CREW_VOTED_OUT


@pytest.mark.parametrize("name", CRC_NAMES)
def test_oracle_matches_the_wide_tagging_crc_streams(oracle_mod, name):
    g = load_golden(os.path.join(WIDE_DIR, name + ".npz"))
    assert g["meta"]["n_agents"] >= 9 and g["crc"].shape == (64, 96)
    got = oracle_crc_stream(oracle_mod, g)
    bad = np.argwhere(got != g["crc"])
    assert bad.size == 0, f"{name}: first mismatch at (seed index, step) = {bad[0].tolist()}"
    assert zlib.crc32(got.tobytes()) == int(g["crc_of_crcs"])


def test_the_fixture_set_is_complete():
    assert CRC_NAMES == ["crc_tagging_1v8_j3_i5", "crc_tagging_2v9_j4_i7_tsr", "crc_tagging_3v9_j8_i4"]
    assert os.path.exists(os.path.join(WIDE_DIR, "directed_tagging12_votes.npz"))


def test_family_lists_tagging_for_three_to_twelve_agents():
    """tools/gen_family.py's committed output: every agent count 3 .. 12 has tagging instantiations, in both action orders, with every
    imposter count the reference accepts (fewer imposters than crew members, at most three), each in a translation unit that exists."""
    hdr = open(os.path.join(ROOT, "sus-net_amd", "csrc", "susnet_family.h")).read()
    rows = {tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), SUSNET_VARIANT_TAGGING, (\d), (\d)\)", hdr)}
    want = {(A, o, n) for A in range(3, 13) for o in (0, 1) for n in (1, 2, 3) if n < A - n}
    assert rows == want
    units = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "sus-net_amd", "csrc", "inst_fam_a*_tag*.hip"))}
    for A in range(3, 13):
        for n, suffix in ((1, ""), (2, "_ni2"), (3, "_ni3")):
            if n < A - n:
                name = f"inst_fam_a{A}_tag{suffix}.hip"
                assert name in units, name
                src = open(os.path.join(ROOT, "sus-net_amd", "csrc", name)).read()
                assert f"SUSNET_FAMILY_INSTANTIATE({A}, SUSNET_VARIANT_TAGGING, 1, {n})" in src and f"SUSNET_FAMILY_INSTANTIATE({A}, SUSNET_VARIANT_TAGGING, 0, {n})" in src
