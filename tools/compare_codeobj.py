#!/usr/bin/env python3
"""Do two builds of libsplat_hip.so run the same instructions?  Disassembles every gfx950 code object of each library (one
per translation unit with device code), pairs the objects that share the most kernels and compares the instruction stream
of every kernel (and every device function that stayed out of line) symbol by symbol.
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


def disassemble(blob):
    """{symbol: [instruction text, ...]} of one code object"""
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


def objects(lib):
    """[(the set of kernel symbols a code object holds, its blob)] over every gfx950 code object of `lib` (one per
    translation unit with device code)"""
    return [(set(codeobj.object_kernels(o)), o) for t, l in codeobj.code_objects(lib).items() if "gfx950" in t for o in l]


def pairs(olds, news):
    """(old blob, new blob) for the objects that share the most kernels, largest overlap first, and what found no partner"""
    by_overlap = sorted(((len(ka & kb), i, j) for i, (ka, _) in enumerate(olds) for j, (kb, _) in enumerate(news) if ka & kb), reverse=True)
    seen_i, seen_j, out = set(), set(), []
    for _, i, j in by_overlap:
        if i not in seen_i and j not in seen_j:
            seen_i.add(i); seen_j.add(j)
            out.append((olds[i][1], news[j][1]))
    lone = [("old", olds[i][0]) for i in range(len(olds)) if i not in seen_i] + [("new", news[j][0]) for j in range(len(news)) if j not in seen_j]
    return out, lone


def main(old, new):
    olds, news = objects(old), objects(new)
    bad = n_syms = n_old = n_new = 0
    paired, lone = pairs(olds, news)
    for which, ks in lone:      # none of its kernels is in an object of the other library that is still free
        print("a code object only in %s: %d kernels (%s ...)" % (which, len(ks), ", ".join(sorted(ks)[:3])))
        bad += 1
    for old_blob, new_blob in paired:
        a, b = disassemble(old_blob), disassemble(new_blob)
        n_syms += len(a); n_old += sum(map(len, a.values())); n_new += sum(map(len, b.values()))
        for s in sorted(set(a) | set(b)):
            if s not in a or s not in b:
                print("only in %s: %s" % ("new" if s in b else "old", s))
                bad += 1
            elif a[s] != b[s]:
                k = next((i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
                print("DIFFERS %s: %d vs %d instructions, first at #%d: %r vs %r" %
                      (s, len(a[s]), len(b[s]), k, a[s][k:k + 1], b[s][k:k + 1]))
                bad += 1
    print("%d code objects in old, %d in new; %d symbols, %d instructions in old, %d in new: %s" %
          (len(olds), len(news), n_syms, n_old, n_new, "IDENTICAL" if not bad else "%d differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
