"""Fixtures of `yak sexchr` (tests/golden/sexchr.json).

make_inputs(dir) writes three sex-chromosome sequences and two haplotype assemblies, regenerated on demand from the seeded splitmix64 stream
of gen_golden_triobin (every machine and version writes the same bytes):
  chrY.fa / chrX.fa / par.fa  Y = Y-only + shared + PAR, X = X-only + shared + PAR, PAR alone: the three loads give a Y-only k-mer
                              flag 1, an X-only one 2, a shared one 3 and a PAR one 7
  hap1.fa / hap2.fa           contigs of X-only, Y-only, shared, PAR and autosomal (in no table) sequence, with substitutions, one contig
                              joined from all of them, one contig over 1 Mb, N runs, lowercase, and the edge records (empty, shorter than
                              k, exactly k, a header with a comment)

Run as a script (where the reference is built, `make -C oracle ref`) it stores, for k = 21 and 41, the md5 of the reference's three tables
(`yak count -k K -t1` of each sequence) and of the reference's `sexchr -t1` output, with the output's text where it is short.
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
GOLDEN = os.path.join(HERE, "golden", "sexchr.json")

SEED = 0x5E8C4
KS = (21, 41)
COUNT_ARGS = []
TABLES = ("chrY", "chrX", "par")
TEXT_MAX = 4096
md5 = T.md5


def pieces():
    r = T.SplitMix64(SEED)
    return {"yonly": bytes(T.rand_seq(r, 40000)), "xonly": bytes(T.rand_seq(r, 80000)), "shared": bytes(T.rand_seq(r, 6000)),
            "par": bytes(T.rand_seq(r, 12000)), "auto": bytes(T.rand_seq(r, 100000))}


def hap(seed, p, own):
    """one haplotype assembly: `own` is the sex-specific piece it mostly carries"""
    r = T.SplitMix64(seed)
    rec = []
    for name in (own, "shared", "par", "auto"):
        s = p[name]
        for i in range(2):
            n = 2000 + r.below(len(s) // 3)
            st = r.below(len(s) - n + 1)
            c = T.mutate(r, s[st:st + n], 0.002)
            rec.append((b"%s_%d" % (name.encode(), i), T.revcomp(c) if i else bytes(c)))
    other = "yonly" if own == "xonly" else "xonly"
    rec.append((b"other", bytes(T.mutate(r, p[other][1000:4000], 0.002))))
    mix = bytearray()
    for name in (own, "par", "auto", "shared", other, own):
        st = r.below(len(p[name]) - 3000)
        mix += p[name][st:st + 3000]
    rec.append((b"mix", bytes(mix)))
    big = bytearray()                     # > 1 Mb
    while len(big) < 1100000:
        name = ("auto", own, "par", "shared")[r.below(4)]
        s = p[name]
        n = 5000 + r.below(20000)
        n = min(n, len(s))
        st = r.below(len(s) - n + 1)
        big += T.mutate(r, s[st:st + n], 0.0005)
    rec.append((b"big", bytes(big)))
    s = p[own]
    nrun = bytearray(s[1000:4000])
    for at, ln in ((100, 1), (700, 30), (1500, 200), (2990, 10)):
        nrun[at:at + ln] = b"N" * ln
    rec.append((b"nruns", bytes(nrun)))
    rec.append((b"lower", p["par"][2000:5000].lower()))
    rec.append((b"empty", b""))
    rec.append((b"short", s[500:505]))
    rec.append((b"exact_k21", s[600:621]))
    rec.append((b"exact_k41", p["par"][700:741]))
    rec.append((b"with_comment", s[5000:7500]))
    out = T.fasta(rec)
    return out.replace(b">with_comment\n", b">with_comment some words\tand a tab\n")


def make_inputs(d):
    """write chrY.fa, chrX.fa, par.fa, hap1.fa and hap2.fa into d; returns {name: path}"""
    p = pieces()
    files = {"chrY.fa": T.fasta([(b"chrY", p["yonly"] + p["shared"] + p["par"])]),
             "chrX.fa": T.fasta([(b"chrX", p["xonly"] + p["shared"] + p["par"])]),
             "par.fa": T.fasta([(b"par", p["par"])]),
             "hap1.fa": hap(SEED + 1, p, "xonly"), "hap2.fa": hap(SEED + 2, p, "yonly")}
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths


def ref_count(yak, k, src, dst):
    subprocess.run([yak, "count", "-k%d" % k] + COUNT_ARGS + ["-t1", "-o", dst, src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)


def ref_sexchr(yak, tabs, hap1, hap2, opts=()):
    return subprocess.run([yak, "sexchr", "-t1"] + list(opts) + list(tabs) + [hap1, hap2], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def main():
    if not os.path.exists(REF_YAK):
        sys.exit("build the reference first: make -C oracle ref")
    out = {"seed": SEED, "count_args": COUNT_ARGS, "inputs": {}, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        p = make_inputs(d)
        out["inputs"] = {n: md5(f) for n, f in sorted(p.items())}
        for k in KS:
            tabs = []
            for t in TABLES:
                tabs.append(os.path.join(d, "%s_k%d.yak" % (t, k)))
                ref_count(REF_YAK, k, p[t + ".fa"], tabs[-1])
            case = {"tables_md5": [md5(t) for t in tabs], "out": {}}
            txt = ref_sexchr(REF_YAK, tabs, p["hap1.fa"], p["hap2.fa"])
            e = {"md5": hashlib.md5(txt).hexdigest(), "bytes": len(txt)}
            if len(txt) <= TEXT_MAX:
                e["text"] = txt.decode()
            case["out"]["hap1.fa+hap2.fa"] = e
            out["cases"]["k%d" % k] = case
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
