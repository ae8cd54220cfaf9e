#!/usr/bin/env python3
"""device_code_digest.py LISTING.s [OTHER.s] -- is the device code of two builds the same, whatever order the compiler emitted the kernels in?

The listing is what `hipcc $(HIPFLAGS) --offload-device-only -S yak_amd/csrc/kernels.hip -o LISTING.s` writes (HIPFLAGS: the Makefile's).  It is cut
into one piece per kernel symbol -- the function's text from its label to its end, and its `.amdhsa_kernel` block with every resource line -- the
compiler's running numbers in local labels and the comments that cite them (`.LBB12_3`, `BB12_3`, `.Lfunc_end12`) are dropped, since they count functions in emission order, and the pieces
are sorted by symbol.  Prints the kernel count and the SHA-256 of the sorted pieces; with two listings, also the symbols that differ, and exits 1
if any does."""
import hashlib
import re
import sys


def pieces(path):
    text, desc, cur = {}, {}, None
    for ln in open(path):
        ln = re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+", r"\1\2", ln.rstrip())
        m = re.match(r"\t\.type\t(\S+),@function", ln)
        if m:
            cur, into = m.group(1), text
        m = re.match(r"\t\.amdhsa_kernel (\S+)", ln)
        if m:
            cur, into = m.group(1), desc
        if cur is not None:
            into.setdefault(cur, []).append(ln)
            if ln.startswith(".Lfunc_end") or ln.startswith("\t.end_amdhsa_kernel"):
                cur = None
    return {s: "\n".join(text.get(s, []) + desc[s]) for s in desc}


def digest(p):
    return hashlib.sha256("\n".join(s + "\n" + p[s] for s in sorted(p)).encode()).hexdigest()


if __name__ == "__main__":
    got = [pieces(a) for a in sys.argv[1:3]]
    for a, p in zip(sys.argv[1:], got):
        print(f"{a}: {len(p)} kernels, sha256 {digest(p)}")
    if len(got) == 2:
        diff = sorted(s for s in set(got[0]) | set(got[1]) if got[0].get(s) != got[1].get(s))
        print("differ:", diff if diff else "none")
        sys.exit(1 if diff else 0)
