#!/usr/bin/env python3
"""Two builds of the library, kernel by kernel (keyed by mangled name): which kernels exist in only one, and for the others whether the
metadata note (registers, spills, private / group segment, kernarg size) and the disassembled instruction stream are equal.  The check of
a refactor that must not touch machine code.  Ignored: where a kernel landed (addresses, encodings, the literal of the add pair behind
s_getpc_b64, the symbol text of branch lines), objdump's `...` for elided zero padding and the s_nop / s_code_end padding behind a
kernel's last instruction.

    python tools/kernel_diff.py OLD.so NEW.so        # exit status 1 when a common kernel differs
"""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sus-net_amd"))
import isa_checks as ic  # noqa: E402


def kernels(lib):
    """mangled name -> (note row, normalised instruction list)"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in ic.code_objects(lib, tmp):
            notes = {k["mangled"]: k for k in ic.parse_notes(obj)}
            cur, pc = None, 0
            for ln in ic.disassemble(obj).splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", ln)
                if m:
                    cur = out.setdefault(m.group(1), (notes[m.group(1)], [])) if m.group(1) in notes else None
                    continue
                ins = ln.split("//")[0].strip()
                if cur is None or not ins or ins == "...":
                    continue
                if ins.startswith("s_getpc_b64"):
                    pc = 3  # the s_add_u32 / s_addc_u32 that follow hold a pc-relative address
                elif pc:
                    pc -= 1
                    if ins.startswith(("s_add_u32", "s_addc_u32")):
                        ins = re.sub(r"0x[0-9a-f]+$|-?\d+$", "PCREL", ins)
                cur[1].append(re.sub(r"\s*<[^>]+>$", "", ins))
    for _, ins in out.values():  # the alignment padding behind a kernel's last instruction: as long as what follows it needs
        while ins and ins[-1].startswith(("s_nop", "s_code_end")):
            ins.pop()
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = ic.demangle(sorted(set(old) | set(new)))
    row = lambda k: " ".join(f"{key}={k[0].get(key)}" for key in ic.NOTE_KEYS.values())
    for tag, a, b in (("only in OLD", old, new), ("only in NEW", new, old)):  # (a changed parameter list is a new mangled name: both rows show)
        for n in sorted(set(a) - set(b)):
            print(f"{tag}: {ic.short_name(names[n])}  [{n}]\n    {row(a[n])} instructions={len(a[n][1])}")
    common = sorted(set(old) & set(new))
    differ = [n for n in common if old[n] != new[n]]
    for n in differ:
        what = ("note " if old[n][0] != new[n][0] else "") + (f"instructions {len(old[n][1])} -> {len(new[n][1])}" if old[n][1] != new[n][1] else "")
        print(f"DIFFERS ({what.strip()}): {ic.short_name(names[n])}  [{n}]\n    old: {row(old[n])}\n    new: {row(new[n])}")
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {len(common)} common: {len(common) - len(differ)} identical, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
