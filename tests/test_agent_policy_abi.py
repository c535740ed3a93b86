"""CPU-only checks of the two calls the SpatialDQN collection path adds (susnet_agent_policy_actions, susnet_state_window_push): the
header as C, the exports, the ABI version (additions only: still 8) and every host-side refusal -- before any launch, on handles without
device buffers.  No kernel is launched here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("susnet_agent_policy_actions", "susnet_state_window_push")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_both_calls_are_declared_exported_and_bound_and_the_abi_version_stays(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    for s in NEW:
        assert s in declared and s in pkg._lib.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int, s
    assert len(lib.susnet_agent_policy_actions.argtypes) == len(lib.susnet_policy_actions.argtypes) == 8
    assert len(lib.susnet_state_window_push.argtypes) == 9
    assert lib.susnet_abi_version() == pkg._lib.ABI_VERSION == 8
    table = header[:header.index("Conventions")]  # the table of reference lines each entry point replaces
    assert re.search(r"susnet_agent_policy_actions\s.*src/train\.py:351-381", table)
    assert re.search(r"susnet_state_window_push\s.*src/train\.py:388-389, 441-445", table)


def test_the_header_compiles_as_c_with_both_prototypes(pkg, tmp_path):
    prog = tmp_path / "protos.c"
    prog.write_text("\n".join([
        '#include <stdio.h>', '#include "susnet.h"',
        "typedef int (*agent_fn)(susnet_env *, const float *, const float *, const susnet_policy_opts *, void *, int32_t, int32_t, void *);",
        "typedef int (*push_fn)(susnet_env *, uint8_t *, int32_t, int32_t, int64_t, const uint8_t *, const uint8_t *, const uint8_t *, void *);",
        "int main(void){ agent_fn a = susnet_agent_policy_actions; push_fn p = susnet_state_window_push; agent_fn b = susnet_policy_actions;",
        '  printf("abi %d %d\\n", SUSNET_ABI_VERSION, a != 0 && p != 0 && b != 0); return 0; }']))
    obj = tmp_path / "protos.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(prog), "-o", str(obj)])


def _handle(L, lib, rng_mode=None, batch=8):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=batch, n_imposters=1, n_crew=2, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                     shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX if rng_mode is None else rng_mode).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


Q_IMP, Q_CREW, OUT = 1 << 20, 2 << 20, 3 << 20  # plausible device addresses, never dereferenced: every call below is refused


def test_agent_policy_actions_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound)

    def refused(field, q_imp=Q_IMP, q_crew=Q_CREW, opts=None, out=OUT, dtype=L.U8, layout=L.LAYOUT_BA, handle=h):
        rc = lib.susnet_agent_policy_actions(handle, q_imp, q_crew, C.byref(opts) if opts is not None else None, out, dtype, layout, None)
        assert rc == L.E_INVALID, (field, rc)
        msg = lib.susnet_last_error()
        assert field in msg, (field, msg)
        return msg

    assert b"susnet_agent_policy_actions" in refused(b"q_imposter", q_imp=None)
    assert b"susnet_agent_policy_actions" in refused(b"actions_out", out=None)
    for bad in (L.F32, L.F64, -1, 7):
        assert b"susnet_agent_policy_actions" in refused(b"dtype", dtype=bad)
    for bad in (2, -1):
        assert b"susnet_agent_policy_actions" in refused(b"layout", layout=bad)
    crew_net = L.PolicyOpts(0.0, 1)
    crew_net.crew_packed = 4 << 20
    assert b"susnet_agent_policy_actions" in refused(b"crew_", opts=crew_net)
    dims = (C.c_int32 * 6)(8, 8, 8, 8, 8, 5)
    crew_dims = L.PolicyOpts(0.0, 1)
    crew_dims.crew_dims = dims
    refused(b"crew_", opts=crew_dims)
    crew_q = L.PolicyOpts(0.0, 0)
    crew_q.crew_q_out = 5 << 20
    refused(b"crew_", opts=crew_q)
    refused(b"epsilon", opts=L.PolicyOpts(1.5, 1))
    refused(b"epsilon", opts=L.PolicyOpts(-0.1, 1))
    refused(b"epsilon", opts=L.PolicyOpts(float("nan"), 1))
    assert lib.susnet_agent_policy_actions(None, Q_IMP, Q_CREW, None, OUT, L.U8, L.LAYOUT_BA, None) == L.E_INVALID
    # a well-formed call on a handle without a bound state is refused too (by the handle's own check: nothing is launched)
    assert lib.susnet_agent_policy_actions(h, Q_IMP, Q_CREW, None, OUT, L.U8, L.LAYOUT_BA, None) != 0
    lib.susnet_destroy(h)
    # the production stream belongs to PHILOX handles: a random crew and exploration on a numpy-tape handle
    tape = _handle(L, lib, rng_mode=L.RNG_TAPE)
    assert b"susnet_agent_policy_actions" in refused(b"PHILOX", q_crew=None, handle=tape)
    refused(b"PHILOX", opts=L.PolicyOpts(0.3, 1), handle=tape)
    lib.susnet_destroy(tape)


def test_state_window_push_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    B = 8
    h = _handle(L, lib, batch=B)
    lay = L.Layout()
    assert lib.susnet_get_layout(h, C.byref(lay)) == 0
    S = lay.obs_raw_size
    assert S > 0
    WIN, OBS, DONE, TRUNC = 1 << 20, 2 << 20, 3 << 20, 4 << 20

    def refused(field, window=WIN, T=2, S_=S, n=B, obs=OBS, done=DONE, truncated=TRUNC):
        assert lib.susnet_state_window_push(h, window, T, S_, n, obs, done, truncated, None) == L.E_INVALID, field
        msg = lib.susnet_last_error()
        assert b"susnet_state_window_push" in msg and field in msg, (field, msg)

    refused(b"T = 0", T=0)
    refused(b"T = 9", T=9)
    refused(b"T = -1", T=-1)
    refused(b"S = %d" % (S + 1), S_=S + 1)
    refused(b"S = 0", S_=0)
    refused(b"n = %d" % (B + 1), n=B + 1)
    refused(b"n = 0", n=0)
    refused(b"n = -8", n=-8)
    refused(b"window", window=None)
    refused(b"obs", obs=None)
    refused(b"done", done=None)
    refused(b"truncated", truncated=None)
    assert lib.susnet_state_window_push(None, WIN, 2, S, B, OBS, DONE, TRUNC, None) == L.E_INVALID
    lib.susnet_destroy(h)
