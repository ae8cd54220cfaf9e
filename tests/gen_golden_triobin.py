"""Fixtures of `yak triobin` (tests/golden/triobin.json).

make_inputs(dir) writes a small trio, regenerated on demand from a seeded splitmix64 stream (no library
generator, so every machine and version writes the same bytes):
  pat.fa / mat.fa  short reads (150 bp, 20x) of two haplotypes, the second one the first at ~1 % SNPs
  child.fa         long reads (2-20 kb) of either haplotype, recombinant reads that switch haplotype
                   mid-read, reads from neither, and edge records (empty, shorter than k, exactly k,
                   N runs, lowercase, IUPAC / U bases, a header with a comment)

Run as a script (where the reference is built, `make -C oracle ref`) it stores, for k = 21 and 41, the md5
of the reference's parental tables and of the reference's `triobin -t1` output for each option set, with the
output's text where it is short (every set but -p).
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_YAK = os.path.join(ROOT, "oracle", "_ref", "yak")
GOLDEN = os.path.join(HERE, "golden", "triobin.json")

SEED = 0x7219B1
GENOME = 100000
KS = (21, 41)
COUNT_ARGS = ["-b22"]                     # parental tables: two-pass count with a bloom filter, as the reference's README does
OPTION_SETS = {"c1d2": ["-c1", "-d2"], "default": [], "r05": ["-r0.5"], "p": ["-p"]}
M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def below(self, n):                   # uniform in [0, n): 64-bit multiply-shift, no modulo bias worth the name
        return (self.next() * n) >> 64

    def chance(self, p):
        return self.next() < int(p * (1 << 64))


def rand_seq(r, n):
    out = bytearray(n)
    for i in range(0, n, 32):
        w = r.next()
        for j in range(min(32, n - i)):
            out[i + j] = b"ACGT"[w >> (2 * j) & 3]
    return out


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def mutate(r, s, rate):
    """substitute each base with probability `rate` by one of the three others"""
    s = bytearray(s)
    for i in range(len(s)):
        if r.chance(rate):
            s[i] = b"ACGT"[(b"ACGT".index(s[i]) + 1 + r.below(3)) & 3]
    return s


def sample(r, hap, n, err):
    st = r.below(len(hap) - n + 1)
    s = mutate(r, hap[st:st + n], err)
    return revcomp(s) if r.below(2) else bytes(s)


def haplotypes():
    r = SplitMix64(SEED)
    h1 = rand_seq(r, GENOME)
    h2 = mutate(r, h1, 0.01)
    return bytes(h1), bytes(h2)


def fasta(records):
    return b"".join(b">" + name + b"\n" + seq + b"\n" for name, seq in records)


def parent_reads(seed, hap, cov=20, length=150, err=0.002):
    r = SplitMix64(seed)
    return fasta((b"r%d" % i, sample(r, hap, length, err)) for i in range(cov * len(hap) // length))


def child_reads(h1, h2):
    r = SplitMix64(SEED + 3)
    rec = []
    for hi, hap in ((1, h1), (2, h2)):
        for i in range(6):
            rec.append((b"h%d_%d" % (hi, i), sample(r, hap, 2000 + r.below(18001), 0.001)))
    for i in range(3):                    # recombinant: one haplotype, then the other from the same coordinate on
        n = 6000 + r.below(10001)
        st = r.below(GENOME - n + 1)
        cut = n // 3 + r.below(n // 3)
        a, b = (h1, h2) if i % 2 == 0 else (h2, h1)
        s = mutate(r, a[st:st + cut] + b[st + cut:st + n], 0.001)
        rec.append((b"recomb_%d" % i, revcomp(s) if i == 1 else bytes(s)))
    for i in range(2):
        rec.append((b"neither_%d" % i, bytes(rand_seq(r, 3000 + r.below(2001)))))
    st = r.below(GENOME - 5000)
    rec.append((b"empty", b""))
    rec.append((b"short", h1[st:st + 5]))
    rec.append((b"exact_k21", h1[st:st + 21]))
    rec.append((b"exact_k41", h2[st:st + 41]))
    nrun = bytearray(h1[st:st + 3000])
    for at, ln in ((100, 1), (700, 30), (1500, 200), (2990, 10)):
        nrun[at:at + ln] = b"N" * ln
    rec.append((b"nruns", bytes(nrun)))
    rec.append((b"lower", h2[st + 1000:st + 4000].lower()))
    iupac = bytearray(h1[st + 500:st + 3500])
    for j, at in enumerate(range(37, 3000, 211)):
        iupac[at] = b"RYKMSWBDHVUu"[j % 12]
    rec.append((b"iupac", bytes(iupac)))
    rec.append((b"with_comment", h2[st + 2000:st + 4500]))
    out = fasta(rec)
    return out.replace(b">with_comment\n", b">with_comment some words\tand a tab\n")


def make_inputs(d):
    """write pat.fa, mat.fa, child.fa into d; returns {name: path}"""
    h1, h2 = haplotypes()
    files = {"pat.fa": parent_reads(SEED + 1, h1), "mat.fa": parent_reads(SEED + 2, h2), "child.fa": child_reads(h1, h2)}
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


TEXT_MAX = 4096                           # outputs up to this size are stored as text, larger ones (-p) by md5 and size only


def expected(entry, got):
    """True if `got` is the stored reference output"""
    return hashlib.md5(got).hexdigest() == entry["md5"] and len(got) == entry["bytes"] and got.decode() == entry.get("text", got.decode())


def ref_triobin(yak, pat, mat, child, opts):
    return subprocess.run([yak, "triobin", "-t1"] + opts + [pat, mat, child], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def ref_count(yak, k, src, dst):
    subprocess.run([yak, "count", "-k%d" % k] + COUNT_ARGS + ["-t1", "-o", dst, src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)


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
                ref_count(REF_YAK, k, p[who + ".fa"], tabs[who])
            case = {"pat_md5": md5(tabs["pat"]), "mat_md5": md5(tabs["mat"]), "out": {}}
            for name, opts in OPTION_SETS.items():
                txt = ref_triobin(REF_YAK, tabs["pat"], tabs["mat"], p["child.fa"], opts)
                case["out"][name] = {"md5": hashlib.md5(txt).hexdigest(), "bytes": len(txt)}
                if len(txt) <= TEXT_MAX:
                    case["out"][name]["text"] = txt.decode()
            out["cases"]["k%d" % k] = case
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
