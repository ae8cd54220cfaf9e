"""Fixtures of `yak trioeval` (tests/golden/trioeval.json).

make_inputs(dir) writes a small trio and two assemblies, regenerated on demand from the seeded splitmix64 stream of
gen_golden_triobin (every machine and version writes the same bytes):
  pat.fa / mat.fa  short reads (150 bp, 20x) of two haplotypes: the second is the first at ~1 % SNPs; the first carries a 6 kb
                   insertion the second lacks, the second a 3 kb one the first lacks (typed runs thousands of positions long)
  asm.fa           contigs of either haplotype (two of them over an insertion), contigs that switch haplotype once or several
                   times, two contigs with errors every few dozen bases (short typed runs), one 1.2 Mb contig joined from
                   haplotype pieces, contigs from neither parent, and the edge records of triobin's child set (empty, shorter
                   than k, exactly k, N runs, lowercase, IUPAC / U bases, a header with a comment)
  neither.fa       contigs from neither parent only: no parent-specific k-mer, so the W / H / N rates are 0 / 0

Run as a script (where the reference is built, `make -C oracle ref`) it stores, for k = 21 and 41, the md5 of the reference's
parental tables and of the reference's `trioeval -t1` output for each assembly and option set, with the output's text where it is short.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import gen_golden_triobin as T

HERE = os.path.dirname(os.path.abspath(__file__))
REF_YAK = T.REF_YAK
GOLDEN = os.path.join(HERE, "golden", "trioeval.json")

SEED = 0x7E0E7A
GENOME = 100000
INS = ((40000, 6000), (70000, 3000))      # (position in the shared coordinates, length): pat's insertion, mat's insertion
KS = (21, 41)
COUNT_ARGS = T.COUNT_ARGS
OPTION_SETS = {"default": [], "e": ["-e"], "F": ["-F"], "n1": ["-n1"], "n5": ["-n5"], "c1d2": ["-c1", "-d2"]}
ASSEMBLIES = ("asm.fa", "neither.fa")
TEXT_MAX = 4096
md5 = T.md5
expected = T.expected


def haplotypes():
    """(pat, mat, base, mat_core): pat = base + pat's insertion, mat = base at ~1 % SNPs + mat's insertion"""
    r = T.SplitMix64(SEED)
    base = bytes(T.rand_seq(r, GENOME))
    core = bytes(T.mutate(r, base, 0.01))
    (p1, l1), (p2, l2) = INS
    pat = base[:p1] + bytes(T.rand_seq(r, l1)) + base[p1:]
    mat = core[:p2] + bytes(T.rand_seq(r, l2)) + core[p2:]
    return pat, mat, base, core


def assembly(pat, mat, base, core):
    r = T.SplitMix64(SEED + 3)
    rec = []
    (p1, l1), (p2, l2) = INS
    for hi, hap, over in ((1, pat, (p1 - 5000, p1 + l1 + 6000)), (2, mat, (p2 - 4000, p2 + l2 + 5000))):
        rec.append((b"h%d_ins" % hi, T.mutate(r, hap[over[0]:over[1]], 0.001)))
        for i in range(3):
            n = 5000 + r.below(25001)
            st = r.below(p1 - n) if hi == 1 else r.below(p2 - n)
            rec.append((b"h%d_%d" % (hi, i), T.mutate(r, hap[st:st + n], 0.001)))
    for i in range(4):                    # switches at shared coordinates (below both insertions): 1, 2, 3 and 4 of them
        n = 12000 + r.below(20001)
        st = r.below(p1 - n)
        cuts = sorted({st + 500 + r.below(n - 1000) for _ in range(i + 1)})
        s, at, hap = bytearray(), st, i % 2
        for c in cuts + [st + n]:
            s += (base, core)[hap][at:c]
            at, hap = c, 1 - hap
        s = T.mutate(r, s, 0.001)
        rec.append((b"switch_%d" % i, T.revcomp(s) if i == 2 else bytes(s)))
    for i, (hap, err) in enumerate(((pat, 0.03), (mat, 0.05))):   # errors every few dozen bases cut the typed runs short: -n matters
        st = r.below(p1 - 10000)
        rec.append((b"noisy_%d" % i, T.mutate(r, hap[st:st + 10000], err)))
    big = bytearray()                     # > 1 Mb: 24 pieces of 50 kb from either haplotype
    for i in range(24):
        hap = (pat, mat)[r.below(2)]
        st = r.below(len(hap) - 50000)
        big += hap[st:st + 50000]
    rec.append((b"big", bytes(big)))
    for i in range(2):
        rec.append((b"neither_%d" % i, bytes(T.rand_seq(r, 3000 + r.below(2001)))))
    st = r.below(p1 - 5000)
    rec.append((b"empty", b""))
    rec.append((b"short", pat[st:st + 5]))
    rec.append((b"exact_k21", pat[st:st + 21]))
    rec.append((b"exact_k41", mat[st:st + 41]))
    nrun = bytearray(pat[st:st + 3000])
    for at, ln in ((100, 1), (700, 30), (1500, 200), (2990, 10)):
        nrun[at:at + ln] = b"N" * ln
    rec.append((b"nruns", bytes(nrun)))
    rec.append((b"lower", mat[st + 1000:st + 4000].lower()))
    iupac = bytearray(pat[st + 500:st + 3500])
    for j, at in enumerate(range(37, 3000, 211)):
        iupac[at] = b"RYKMSWBDHVUu"[j % 12]
    rec.append((b"iupac", bytes(iupac)))
    rec.append((b"with_comment", mat[st + 2000:st + 4500]))
    out = T.fasta((n, bytes(s)) for n, s in rec)
    return out.replace(b">with_comment\n", b">with_comment some words\tand a tab\n")


def neither():
    r = T.SplitMix64(SEED + 4)
    return T.fasta([(b"n%d" % i, bytes(T.rand_seq(r, 2000 + r.below(4001)))) for i in range(3)] + [(b"n_empty", b"")])


def make_inputs(d):
    """write pat.fa, mat.fa, asm.fa, neither.fa into d; returns {name: path}"""
    pat, mat, base, core = haplotypes()
    files = {"pat.fa": T.parent_reads(SEED + 1, pat), "mat.fa": T.parent_reads(SEED + 2, mat), "asm.fa": assembly(pat, mat, base, core),
             "neither.fa": neither()}
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths


def ref_trioeval(yak, pat, mat, fa, opts):
    return subprocess.run([yak, "trioeval", "-t1"] + opts + [pat, mat, fa], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def main():
    if not os.path.exists(REF_YAK):
        sys.exit("build the reference first: make -C oracle ref")
    out = {"seed": SEED, "genome": GENOME, "count_args": COUNT_ARGS, "option_sets": OPTION_SETS, "inputs": {}, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        p = make_inputs(d)
        out["inputs"] = {n: md5(f) for n, f in sorted(p.items())}
        for k in KS:
            tabs = {}
            for who in ("pat", "mat"):
                tabs[who] = os.path.join(d, "%s_k%d.yak" % (who, k))
                T.ref_count(REF_YAK, k, p[who + ".fa"], tabs[who])
            case = {"pat_md5": md5(tabs["pat"]), "mat_md5": md5(tabs["mat"]), "out": {}}
            for fa in ASSEMBLIES:
                for name, opts in OPTION_SETS.items():
                    txt = ref_trioeval(REF_YAK, tabs["pat"], tabs["mat"], p[fa], opts)
                    e = {"md5": hashlib.md5(txt).hexdigest(), "bytes": len(txt)}
                    if len(txt) <= TEXT_MAX:
                        e["text"] = txt.decode()
                    case["out"]["%s:%s" % (fa, name)] = e
            out["cases"]["k%d" % k] = case
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
