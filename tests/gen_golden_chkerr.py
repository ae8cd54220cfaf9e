"""Fixtures of `yak chkerr` (tests/golden/chkerr.json).

make_inputs(dir) writes a genome's reads and an assembly of it, regenerated on demand from the seeded splitmix64 stream of
gen_golden_triobin (every machine and version writes the same bytes):
  reads.fa   short reads (150 bp, 20x) of a 100 kb genome; reads that start in THIN are kept one time in twelve, so the k-mers there
             have counts of 1-2 and -c decides whether they are low
  asm.fa     contigs of the genome with isolated substitutions (streaks of about k low k-mers), small insertions and deletions, a
             foreign insert of several hundred bp, the thinned region, foreign bases at a contig's start and end, N runs, lowercase, one
             contig over 1 Mb (ten copies of the genome at a low substitution rate), and the edge records (empty, shorter than k, exactly
             k, a header with a comment)

Run as a script (where the reference is built, `make -C oracle ref`) it stores, for k = 21 and 41, the md5 of the reference's table
(`yak count -k K -t1`, one pass: singletons kept) and of the reference's `chkerr -t1` output for each option set, with the output's text
where it is short.
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
GOLDEN = os.path.join(HERE, "golden", "chkerr.json")

SEED = 0xC4E77
GENOME = 100000
THIN = (60000, 64000)
KS = (21, 41)
COUNT_ARGS = []                           # one pass, no bloom filter: k-mers seen once stay in the table with count 1
OPTION_SETS = {"default": [], "c1": ["-c1"], "c0": ["-c0"], "c1024": ["-c1024"], "s0": ["-s0"], "sm1": ["-s-1"], "s100": ["-s100"],
               "c1s0": ["-c1", "-s0"]}
TEXT_MAX = 4096
md5 = T.md5
expected = T.expected


def genome():
    return bytes(T.rand_seq(T.SplitMix64(SEED), GENOME))


def reads(g):
    r = T.SplitMix64(SEED + 1)
    rec = []
    for i in range(20 * GENOME // 150):
        st = r.below(GENOME - 150 + 1)
        s = T.mutate(r, g[st:st + 150], 0.002)
        s = T.revcomp(s) if r.below(2) else bytes(s)
        if THIN[0] - 150 < st < THIN[1] and r.below(12) != 0:
            continue
        rec.append((b"r%d" % i, s))
    return T.fasta(rec)


def substitute(s, at):
    s = bytearray(s)
    for p in at:
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1) & 3]
    return bytes(s)


def assembly(g):
    r = T.SplitMix64(SEED + 2)
    rec = []
    rec.append((b"subs", substitute(g[5000:25000], range(700, 20000, 1900))))
    ind = bytearray(g[25000:40000])                       # from the end, so that earlier positions stay put
    for at, op in ((12000, b"-3"), (9000, b"+2"), (6000, b"-1"), (3000, b"+7"), (1000, b"-12")):
        n = int(op[1:])
        if op[:1] == b"-":
            del ind[at:at + n]
        else:
            ind[at:at] = T.rand_seq(r, n)
    rec.append((b"indels", bytes(ind)))
    rec.append((b"foreign", g[40000:45000] + bytes(T.rand_seq(r, 600)) + g[45000:50000]))
    rec.append((b"thin", g[THIN[0] - 3000:THIN[1] + 3000]))
    rec.append((b"ends", bytes(T.rand_seq(r, 80)) + g[70000:76000] + bytes(T.rand_seq(r, 50))))
    rec.append((b"clean", T.revcomp(g[80000:90000])))
    nrun = bytearray(substitute(g[10000:13000], (400, 1480, 2400)))
    for at, ln in ((100, 1), (700, 30), (1500, 200), (2990, 10)):
        nrun[at:at + ln] = b"N" * ln
    rec.append((b"nruns", bytes(nrun)))
    rec.append((b"lower", substitute(g[30000:33000], (1200,)).lower()))
    big = bytearray()                     # > 1 Mb
    for i in range(10):
        big += T.mutate(r, g, 0.0002)
    rec.append((b"big", bytes(big)))
    rec.append((b"empty", b""))
    rec.append((b"short", g[500:505]))
    rec.append((b"exact_k21", substitute(g[600:621], (10,))))
    rec.append((b"exact_k41", g[700:741]))
    rec.append((b"with_comment", substitute(g[50000:52500], (1000,))))
    rec.append((b"foreign_only", bytes(T.rand_seq(r, 300))))
    out = T.fasta(rec)
    return out.replace(b">with_comment\n", b">with_comment some words\tand a tab\n")


def make_inputs(d):
    """write reads.fa and asm.fa into d; returns {name: path}"""
    g = genome()
    files = {"reads.fa": reads(g), "asm.fa": assembly(g)}
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths


def ref_count(yak, k, src, dst):
    subprocess.run([yak, "count", "-k%d" % k] + COUNT_ARGS + ["-t1", "-o", dst, src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)


def ref_chkerr(yak, tab, fa, opts):
    return subprocess.run([yak, "chkerr", "-t1"] + opts + [tab, fa], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def main():
    if not os.path.exists(REF_YAK):
        sys.exit("build the reference first: make -C oracle ref")
    out = {"seed": SEED, "genome": GENOME, "count_args": COUNT_ARGS, "option_sets": OPTION_SETS, "inputs": {}, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        p = make_inputs(d)
        out["inputs"] = {n: md5(f) for n, f in sorted(p.items())}
        for k in KS:
            tab = os.path.join(d, "reads_k%d.yak" % k)
            ref_count(REF_YAK, k, p["reads.fa"], tab)
            case = {"table_md5": md5(tab), "out": {}}
            for name, opts in OPTION_SETS.items():
                txt = ref_chkerr(REF_YAK, tab, p["asm.fa"], opts)
                e = {"md5": hashlib.md5(txt).hexdigest(), "bytes": len(txt)}
                if len(txt) <= TEXT_MAX:
                    e["text"] = txt.decode()
                case["out"]["asm.fa:%s" % name] = e
            out["cases"]["k%d" % k] = case
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
