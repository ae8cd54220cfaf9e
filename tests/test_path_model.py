"""The sequential model of the path kernels (tests/tools/path_model_check.cpp: the staging, the claims of every node in the index, the hits, the count
per tile, the scan of the tile array, the emit and the tallies with the very functions of yak_amd/path/path_step.h, the texts of path_text.h, the
reader of yak_amd/layer/seq_reader.h; built with the host compiler under the address and undefined-behaviour sanitizers and run as a program of its own, nothing
of it is loaded into Python) against the restatement of tests/path_util.py, byte for byte: the hits, the records, the GAF and the -s text -- on the
hand-derived cases of tests/test_path.py, on tiny random tables, with tiles of 8 and of 1024 positions, at a capacity of the index equal to the
number of its keys, where the probe walks are longest; its refusals; and its reader against the engine's on the golden inputs, and in its two
modes -- the quality kept or only counted -- on awkward files."""
import glob
import gzip
import os
import random
import shutil
import subprocess

import pytest

import graph_util as U
import path_util as P
import walk_util as W
from conftest import ROOT
from test_gfa import table_of
from test_path import BUBBLE, restated

HAND = {
    "bubble": (5, BUBBLE, [b"TTCAGGTCTCATG", b"TTCAGGACTCATG", b"CATGAGACCTGAA", b"TCAGGTC"]),
    "tip": (5, ["TTCAGGACTCATG", "CAGGAGG"], [b"TTCAGGAGG", b"CCTCCTGAA"]),
    "cycle": (5, ["AC" * 6], [b"AC" * 6, b"GT" * 6, b"AC" * 40]),
    "hairpin": (5, ["ACGT" * 4], [b"ACGTACGTAC"]),
    "letters": (5, BUBBLE, [b"TTCAGGNCTCATG", b"TTCA", b"GGGGGGGG", b"ttcaggucucaug", b""]),
    "lone": (5, ["AACCG"], [b"AACCG", b"CGGTT", b"AACCGG"]),
    "cycle_and_open": (5, ["AC" * 6, "AAGGT"], [b"ACACACAAGGT", b"ACCTT"]),
}
EVERY = ["".join("ACGT"[i >> 2 * j & 3] for j in range(5)) for i in range(1024)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the model with the kernels' tiles of 1024 positions, and with tiles of 8"""
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++ on the path: the model of the kernels cannot be built"
    d = tmp_path_factory.mktemp("path")
    out = {}
    for tile, defs in ((1024, []), (8, ["-DPX_THREADS_N=2"])):
        out[tile] = str(d / ("path_model_check_%d" % tile))
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + defs +
                       [os.path.join(ROOT, "tests", "tools", "path_model_check.cpp"), "-o", out[tile], "-lz"], check=True, capture_output=True, text=True)
    return out


def run(program, fn, fa, mode):
    r = subprocess.run([program, fn, fa, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def model_equals(programs, d, name, k, seqs, reads, min_cnt=1, caps=(0,), tiles=(1024, 8), min_len=0):
    """the four outputs of the model at every capacity of caps (0: the default; -1: the number of keys) and every tile size; returns the
    restatement and the longest probes"""
    r = restated(seqs, k, reads, min_cnt)
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, min_cnt)
    amap, desc, bases = W.restate(k, recs, min_cnt, r["ug"])
    names = ["r%d" % i for i in range(len(reads))]
    fa = str(d / (name + ".fa"))
    open(fa, "wb").write(P.fasta(names, reads))
    n_key, probes = sum(u[1] for u in r["ug"]), []
    for cap in caps:
        fn = str(d / ("%s_c%d_s%d.pxm" % (name, min_cnt, cap)))
        P.model_file(fn, k, min_cnt, n_key if cap < 0 else cap, min_len, desc, bases)
        for tile in tiles:
            prog = programs[tile]
            assert run(prog, fn, fa, "hits") == "".join("%d\n" % h for h in r["hits"]).encode()
            body, last = run(prog, fn, fa, "records").rsplit(b"T ", 1)
            assert body == P.records_text(r["paths"], r["steps"], r["tally"])
            slots, keys, probe = (int(v) for v in last.split())
            want = n_key if cap < 0 else cap
            assert keys == n_key and slots & (slots - 1) == 0 and (slots >= 2 * n_key if not want else want <= slots < 2 * max(want, 1)) and probe <= slots
            probes.append(probe)
            assert run(prog, fn, fa, "gaf") == P.gaf_text(k, r["ug"], names, r["lens"], r["paths"], r["steps"], min_len)
            assert run(prog, fn, fa, "stats") == r["stats"].encode()
    return r, probes


def test_model_on_the_hand_cases(programs, tmp_path):
    for name, (k, seqs, reads) in sorted(HAND.items()):
        for min_cnt in (1, 2):
            model_equals(programs, tmp_path, name, k, seqs, reads, min_cnt, caps=(0, -1))
    r, _ = model_equals(programs, tmp_path, "filter", 5, BUBBLE, HAND["letters"][2], min_len=7)
    assert len(r["paths"]) == 3
    r, _ = model_equals(programs, tmp_path, "none", 5, ["AACCG"], [b"AACCG", b"AACCGAACCG"], min_cnt=2)      # a table without a node
    assert r["ug"] == [] and r["tally"] == [(1, 0, 0, 0), (6, 0, 0, 0)]
    r, _ = model_equals(programs, tmp_path, "noseq", 5, BUBBLE, [])                                            # no sequence, no position
    assert r["paths"] == []


def test_model_at_a_full_table(programs, tmp_path):
    """512 unitigs of one node: 512 keys in 512 slots, no free slot left -- every claim and every look-up still ends, the longest after many slots"""
    rng = random.Random(9)
    reads = ["".join(rng.choice("ACGT") for _ in range(40)).encode() for _ in range(20)]
    r, probes = model_equals(programs, tmp_path, "full", 5, EVERY, reads, caps=(0, -1, 600), tiles=(1024,))
    assert all(t[0] == t[1] == 36 for t in r["tally"]) and probes[0] < 32 < probes[1] and probes[2] <= probes[1]


def test_model_on_tiny_random_tables(programs, tmp_path):
    rng = random.Random(6)
    n_path = 0
    for it in range(40):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        reads = P.reads_of(rng, seqs, 8, 1, 30, sub=0.05, n_rate=0.03, mixed_case=True) + [s.encode() for s in seqs]
        r, _ = model_equals(programs, tmp_path, "t%d" % it, k, seqs, reads, rng.choice((1, 1, 2)), caps=(0, -1), tiles=(8,) if it % 4 else (1024, 8))
        n_path += len(r["paths"])
    assert n_path > 300


def test_model_across_tiles_at_k31(programs, tmp_path):
    """a genome of 3000 bases at k = 31: one unitig over three tiles of its bases; reads on both strands with substitutions and Ns, a read of the
    whole genome over three tiles of the image, and paths that start and end around every tile edge"""
    rng = random.Random(31)
    g = "".join(rng.choice("ACGT") for _ in range(3000))
    reads = P.reads_of(rng, [g], 30, 20, 120, sub=0.02, n_rate=0.005, mixed_case=True) + [g.encode(), P.rc_bytes(g.encode())]
    r, _ = model_equals(programs, tmp_path, "g3000", 31, [g], reads, caps=(0, -1))
    assert len(r["ug"]) == 1 and r["tally"][-1] == (2970, 2970, 1, 1) and r["paths"][-1]["ps"] == 0 and any(t[2] >= 2 for t in r["tally"])


def test_model_refuses(programs, tmp_path):
    """a capacity below the number of keys, and descriptors that do not fit the bases: a message, not a walk without end or a read outside"""
    k, seqs, reads = HAND["bubble"]
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, 1)
    ug = U.unitigs(k, recs, 1)
    amap, desc, bases = W.restate(k, recs, 1, ug)
    fa = str(tmp_path / "r.fa")
    open(fa, "wb").write(P.fasta(["r"], reads[:1]))
    n_key = sum(u[1] for u in ug)
    for name, cap, dd, bb, what in (("small", n_key - 1, desc, bases, b"below the number of keys"),
                                    ("off", 0, [desc[0], (desc[1][0] + 1,) + desc[1][1:]] + desc[2:], bases, b"does not fit"),
                                    ("long", 0, desc[:-1] + [(desc[-1][0], desc[-1][1] + 1) + desc[-1][2:]], bases, b"does not fit"),
                                    ("huge", 0, [(desc[0][0], (1 << 64) - 2) + desc[0][2:]] + desc[1:], bases, b"does not fit"),
                                    ("short", 0, desc, bases[:-1], b"does not fit"),
                                    ("nobase", 0, desc, bases[:3] + b"N" + bases[4:], b"does not fit"),
                                    ("twice", 0, desc, bases[:9] + bases[:9] + bases[18:], b"two places")):
        for tile in (1024, 8):
            fn = str(tmp_path / (name + ".pxm"))
            P.model_file(fn, k, 1, cap, 0, dd, bb)
            r = subprocess.run([programs[tile], fn, fa, "gaf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            assert r.returncode == 1 and r.stdout == b"" and what in r.stderr, (name, r.stderr)


def test_reader_against_the_engines(programs, tmp_path):
    """what SeqReader gives, sequence after sequence, is the image the engine's reader makes of the same file: the golden inputs, plain and gzip, a FASTQ
    with '@' and '+' at the start of quality lines, and line ends of \\r\\n"""
    import yak_amd
    fq = tmp_path / "tricky.fq"
    fq.write_bytes(b"@a first\nACGTAC\nGTNN\n+\n@@@@@@\n++++\n@b\tx\nTTGCA\n+b\n+@+@+\n>c\r\nAC\r\nGT\r\n>d\n>e\nA\n")
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "inputs", "*"))) + [str(fq)]
    assert len(files) >= 4
    for f in list(files):
        gz = str(tmp_path / (os.path.basename(f) + ".gz"))
        with gzip.open(gz, "wb") as o:
            o.write(open(f, "rb").read())
        files.append(gz)
    for f in files:
        got = run(programs[1024], "-", f, "reader")
        seqs = [ln.split(b"\t", 1)[1] for ln in got.split(b"\n")[:-1]]
        img = yak_amd.host_image(f, 0, fast=False)
        assert b"".join(s + b"\n" for s in seqs) == img, f
    got = run(programs[1024], "-", str(fq), "reader")
    assert got == b"a\tACGTACGTNN\nb\tTTGCA\nc\tACGT\nd\t\ne\tA\n"


AWKWARD = [   # what the file holds, and the record it is: name, comment, sequence, quality
    (b"@r1 first comment\r\nACGT\r\nAC\r\n+\r\nIIII\r\nJJ\r\n", (b"r1", b"first comment", b"ACGTAC", b"IIIIJJ")),      # \r\n; sequence and quality over two lines
    (b"\n\n>r2\tc\tx\n\nAC\n\nGT\n", (b"r2", b"c\tx", b"ACGT", b"")),                                                  # empty lines in front and inside
    (b">\nAAA\n", (b"", b"", b"AAA", b"")),                                                                            # an empty name
    (b"> only a comment\nCC\n", (b"", b"only a comment", b"CC", b"")),
    (b">e\n", (b"e", b"", b"", b"")),                                                                                  # an empty sequence
    (b"@q\nAC\nGT\n+q\n@+\n>@\n", (b"q", b"", b"ACGT", b"@+>@")),                                                      # quality lines that start like headers
    (b"@z\n+\n", (b"z", b"", b"", b"")),
    (b">last trailing \nACGT", (b"last", b"trailing ", b"ACGT", b"")),                                                 # no newline at the end
]


def kept_records(out):
    """the records of the mode records-kept: four times `<length>:<bytes>`, then a newline"""
    recs, at = [], 0
    while at < len(out):
        rec = []
        for _ in range(4):
            colon = out.index(b":", at)
            n = int(out[at:colon])
            rec.append(out[colon + 1:colon + 1 + n])
            at = colon + 1 + n
        assert out[at:at + 1] == b"\n"
        at += 1
        recs.append(tuple(rec))
    return recs


def test_reader_keeps_or_counts_the_quality(programs, tmp_path):
    """SeqReader in its two modes on one set of awkward files, plain and gzip: \\r\\n, a sequence and a quality over several lines, empty lines, no
    newline at the end, an empty name, a comment, an empty sequence -- and behind them a record whose quality is one character short, which ends the
    file in front of that record, whether more follows it or not.  With the quality kept the four parts of every record are what was written; with
    it counted the names, the sequences and the number of records are the same"""
    want = [rec for _, rec in AWKWARD]
    whole = b"".join(text for text, _ in AWKWARD)
    files = {"whole.fq": whole, "short.fq": whole + b"\n@bad\nACGT\n+\nIII\n>after\nAC\n", "short_at_end.fq": whole + b"\n@bad\nACGT\n+\nIII"}
    for name, text in sorted(files.items()):
        assert len(text) < 400
        plain, gz = tmp_path / name, tmp_path / (name + ".gz")
        plain.write_bytes(text)
        with gzip.open(gz, "wb") as o:
            o.write(text)
        for f in (str(plain), str(gz)):
            kept = kept_records(run(programs[1024], "-", f, "records-kept"))
            assert kept == want, f
            counted = run(programs[1024], "-", f, "reader")
            assert counted == b"".join(r[0] + b"\t" + r[2] + b"\n" for r in kept), f
