"""CPU-only checks of the feature-window call (susnet_window_push): the header as C, the struct against its ctypes mirror, the export, the
ABI version (an addition only: still 8) and the host-side refusals -- every one before any launch, on a handle without device buffers.
No kernel is launched here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_window_io_matches_the_header_compiled_as_c(pkg, tmp_path):
    L = pkg._lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "susnet.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(susnet_window_io));']
    for fname, _ in L.WindowIO._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(susnet_window_io, {fname}));')
    lines += ['printf("abi %d\\n", SUSNET_ABI_VERSION);', 'printf("max_f %d\\n", SUSNET_MLP_MAX_F);', "return 0;}"]
    prog = tmp_path / "window_io.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "window_io"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(L.WindowIO)
    assert [f for f, _ in L.WindowIO._fields_] == ["fresh", "done", "truncated", "src", "dst", "T", "F", "n"]
    for fname, _ in L.WindowIO._fields_:
        assert int(out[fname]) == getattr(L.WindowIO, fname).offset, fname
    assert int(out["abi"]) == L.ABI_VERSION == 8
    assert int(out["max_f"]) == L.MLP_MAX_F


def test_window_push_is_declared_and_exported_and_the_abi_version_stays(pkg):
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    declared = set(re.findall(r"\b(susnet_[a-z_]+)\s*\(", header))
    lib = pkg._lib.lib()
    assert "susnet_window_push" in declared and "susnet_window_push" in pkg._lib.EXPORTS and hasattr(lib, "susnet_window_push")
    assert lib.susnet_abi_version() == pkg._lib.ABI_VERSION == 8
    doc = header[header.index("one tick on.  The reference keeps"):header.index("typedef struct susnet_window_io")]
    for cite in ("318-322", "388-389", "441-445", "OUT OF PLACE"):  # the reference's window rules are cited where the call is declared
        assert cite in doc, cite


def _handle(L, lib):
    cfg = L.Config()
    cfg.struct_bytes, cfg.abi_version = C.sizeof(L.Config), L.ABI_VERSION
    for k, v in dict(variant=L.VARIANT_BASE, batch=8, n_imposters=1, n_crew=2, n_jobs=4, grid_n=9, max_time_steps=1000, is_action_order_random=1,
                     shuffle_imposter_index=1, tag_reset_interval=50, rng_mode=L.RNG_PHILOX).items():
        setattr(cfg, k, v)
    for i in range(cfg.grid_n):
        cfg.grid_rows[i] = (1 << cfg.grid_n) - 1
    h = C.c_void_p()
    assert lib.susnet_create(C.byref(cfg), C.byref(h)) == 0, lib.susnet_last_error()
    return h


def _io(L, T=2, F=36, n=5, fresh=1 << 20, src=2 << 20, dst=3 << 20, done=4 << 20, truncated=5 << 20):
    """A well-formed susnet_window_io whose pointers are plausible, aligned, disjoint, never dereferenced values (the calls below are all
    refused)."""
    io = L.WindowIO()
    io.T, io.F, io.n = T, F, n
    io.fresh, io.src, io.dst, io.done, io.truncated = fresh, src, dst, done, truncated
    return io


def test_window_push_refusals_name_the_field(pkg):
    L = pkg._lib
    lib = L.lib()
    h = _handle(L, lib)  # (no state blob is bound: the call needs none)

    def refused(io, field):
        assert lib.susnet_window_push(h, C.byref(io), None) == L.E_INVALID, field
        msg = lib.susnet_last_error()
        assert b"susnet_window_push" in msg and field in msg, (field, msg)

    refused(_io(L, T=0), b"T = 0")
    refused(_io(L, T=9), b"T = 9")
    refused(_io(L, T=-1), b"T = -1")
    refused(_io(L, F=0), b"F = 0")
    refused(_io(L, T=5, F=205), b"T * F = 1025")
    refused(_io(L, T=1, F=1025), b"T * F = 1025")
    refused(_io(L, T=8, F=1 << 29), b"T * F")  # (the product does not wrap in 32 bits)
    refused(_io(L, n=0), b"n = 0")
    refused(_io(L, n=-3), b"n = -3")
    refused(_io(L, fresh=None), b"fresh")
    refused(_io(L, src=None), b"src")
    refused(_io(L, dst=None), b"dst")
    refused(_io(L, fresh=(1 << 20) + 2), b"fresh")
    refused(_io(L, src=(2 << 20) + 1), b"src")
    refused(_io(L, dst=(3 << 20) + 3), b"dst")
    refused(_io(L, dst=2 << 20), b"dst overlaps src")                       # dst == src: in place
    T, F, n = 2, 36, 5
    tail = (2 << 20) + (n * T * F - 1) * 4                                  # src's last dword
    refused(_io(L, T=T, F=F, n=n, dst=tail), b"dst overlaps src")           # dst starts on src's tail
    refused(_io(L, T=T, F=F, n=n, dst=(2 << 20) - (n * T * F - 1) * 4), b"dst overlaps src")  # dst's tail on src's first dword
    refused(_io(L, T=T, F=F, n=n, dst=(1 << 20) + 8), b"dst overlaps fresh")
    assert lib.susnet_window_push(None, C.byref(_io(L)), None) == L.E_INVALID
    assert lib.susnet_window_push(h, None, None) == L.E_INVALID
    lib.susnet_destroy(h)
