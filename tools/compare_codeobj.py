#!/usr/bin/env python3
"""Do two builds of libsplat_hip.so run the same instructions?  Disassembles the gfx950 code object of each library and
compares the instruction stream of every kernel (and every device function that stayed out of line) symbol by symbol.
The order of the symbols in the object and their addresses do not matter; one changed instruction does.

    python tools/compare_codeobj.py OLD.so NEW.so          # exit 0: identical, 1: a difference (listed)

For changes that claim to move code without changing it (a refactor, a lifted function)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def streams(lib):
    """{symbol: [instruction text, ...]} of the gfx950 code object of `lib`"""
    blob = next(o for t, l in codeobj.code_objects(lib).items() if "gfx950" in t for o in l)
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(blob)
        f.flush()
        out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
    syms, cur = {}, None
    for ln in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif ln.startswith("\t") and cur is not None:
            # the comment holds the address (and a branch's absolute target): position, not instruction
            cur.append(ln.split("//")[0].strip())
    return syms


def main(old, new):
    a, b = streams(old), streams(new)
    bad = 0
    for s in sorted(set(a) | set(b)):
        if s not in a or s not in b:
            print("only in %s: %s" % ("new" if s in b else "old", s))
            bad += 1
        elif a[s] != b[s]:
            k = next((i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
            print("DIFFERS %s: %d vs %d instructions, first at #%d: %r vs %r" %
                  (s, len(a[s]), len(b[s]), k, a[s][k:k + 1], b[s][k:k + 1]))
            bad += 1
    print("%d symbols, %d instructions in old, %d in new: %s" %
          (len(a), sum(map(len, a.values())), sum(map(len, b.values())), "IDENTICAL" if not bad else "%d differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
