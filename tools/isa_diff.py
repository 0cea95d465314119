"""Compare the gfx950 code of two builds of a HIP shared library, kernel by kernel.

    python tools/isa_diff.py LIB_A LIB_B [--require-identical REGEX] [--same-as OLD=NEW]...

Every gfx950 code object of each library is disassembled (llvm-objdump, no raw bytes, no
addresses, comments stripped) and split per symbol.  For every symbol the instruction
streams are compared as text: `identical`, or `differs (nA -> nB instructions)`, with the
kernel's entry of isa_hazards.kernel_resources() (VGPRs, spilled VGPRs, scratch bytes) in
both builds beside it.  Exit 1 if a symbol matching --require-identical differs or is
missing from one build (a refactor that must not move the hot kernels' code: build the
parent with tools/mk_variant.sh prev, then compare).

--same-as OLD=NEW (repeatable; the symbols as llvm-objdump prints them): symbol OLD of build A
is compared with symbol NEW of build B under the same rule, for a kernel whose name or
argument types changed, or whose work another kernel took over.  A pair that is not
identical fails the run; OLD may then be missing from B, and NEW from A, without failing it.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile

from isa_hazards import LLVM, code_objects, kernel_resources

SYMBOL = re.compile(r"^[0-9a-f]* ?<([^>]+)>:$")


def functions(lib: str):
    """{symbol: [instruction lines]} over the gfx950 code objects of lib."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", "--no-show-raw-insn",
                                   "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in text.splitlines():
                s = line.split("//")[0].strip()
                m = SYMBOL.match(s)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif s and s != "..." and cur is not None:   # "...": zero padding after a function, no instruction
                    cur.append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--require-identical", metavar="REGEX", default=None)
    ap.add_argument("--same-as", metavar="OLD=NEW", action="append", default=[])
    a = ap.parse_args()
    pairs = [tuple(p.split("=", 1)) for p in a.same_as]
    paired = {old for old, _ in pairs} | {new for _, new in pairs}
    fa, fb = functions(a.lib_a), functions(a.lib_b)
    ra, rb = kernel_resources(a.lib_a), kernel_resources(a.lib_b)
    need = re.compile(a.require_identical) if a.require_identical else None
    same = differ = failed = 0
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            verdict = "only in " + ("A" if name in fa else "B")
        elif fa[name] == fb[name]:
            verdict = "identical"
        else:
            verdict = f"differs ({len(fa[name])} -> {len(fb[name])} instructions)"
        ok = verdict == "identical"
        same += ok
        differ += not ok
        res = ""
        if name in ra or name in rb:
            res = f"  (vgpr, spilled, scratch) A {ra.get(name)} B {rb.get(name)}"
        required = bool(need and need.search(name)) and not (name in paired and verdict.startswith("only in"))
        failed += required and not ok
        print(f"{name}: {verdict}{res}{'  [required identical]' if required and not ok else ''}")
    for old, new in pairs:
        if old not in fa or new not in fb:
            verdict = "missing: " + (f"{old} from A" if old not in fa else f"{new} from B")
        elif fa[old] == fb[new]:
            verdict = "identical"
        else:
            verdict = f"differs ({len(fa[old])} -> {len(fb[new])} instructions)"
        failed += verdict != "identical"
        print(f"A {old} same as B {new}: {verdict}  (vgpr, spilled, scratch) A {ra.get(old)} B {rb.get(new)}")
    print(f"{same} identical, {differ} not; {sum(map(len, fa.values()))} -> {sum(map(len, fb.values()))} instructions")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
