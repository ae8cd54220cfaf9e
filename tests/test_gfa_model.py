"""The sequential model of the link kernels (tests/tools/gfa_model_check.cpp: the claims in the end table, the count of every oriented end, the scan
and the emit with the very functions of yak_amd/gfa/gfa_step.h, the texts of gfa_text.h; built with the host compiler under the address and
undefined-behaviour sanitizers and run as a program of its own, nothing of it is loaded into Python) against the restatement of tests/gfa_util.py,
byte for byte: the GFA, the -s text and the links -- on the hand-derived cases of tests/test_gfa.py, on tiny random tables, on reads, and at a
capacity of the end table equal to the number of its keys, where the probe walks are longest."""
import os
import random
import shutil
import subprocess

import pytest

import gfa_util as G
import graph_util as U
import walk_util as W
from conftest import ROOT
from test_gfa import table_of

HAND = {
    "polya": (5, ["A" * 9]), "hairpin": (5, ["ACGT" * 4]), "ac": (5, ["AC" * 6]), "acg": (5, ["ACG" * 5]), "lone": (5, ["AACCG"]), "lone_hairpin": (5, ["AACGT"]),
    "bubble": (5, ["TTCAGGACTCATG", "TTCAGGTCTCATG"]), "tip": (5, ["TTCAGGACTCATG", "CAGGAGG"]), "cycle_and_open": (5, ["AC" * 6, "AAGGT"]),
    "every_5_mer": (5, ["".join("ACGT"[i >> 2 * j & 3] for j in range(5)) for i in range(1024)]),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++ on the path: the model of the kernels cannot be built"
    exe = str(tmp_path_factory.mktemp("gfa") / "gfa_model_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tools", "gfa_model_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(program, fn, mode):
    r = subprocess.run([program, fn, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def model_equals(program, d, name, k, x, c, min_cnt, caps=(0,)):
    """the three outputs of the model at every capacity of caps (0: the default; -1: the number of keys); returns (unitigs, links, longest probes)"""
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    amap, desc, bases = W.restate(k, recs, min_cnt, ug)
    links = G.links_by_strings(k, ug)
    assert links == G.links_by_map(k, recs, min_cnt, ug, amap)
    n_key, probes = G.n_keys(ug), []
    for cap in caps:
        fn = str(d / ("%s_c%d_s%d.gfm" % (name, min_cnt, cap)))
        G.model_file(fn, k, min_cnt, n_key if cap < 0 else cap, st, ug, desc, bases)
        assert run(program, fn, "gfa") == G.gfa_text(k, ug, links)
        assert run(program, fn, "stats") == G.stats_text(k, min_cnt, st, ug, links)
        body, last = run(program, fn, "links").rsplit(b"T ", 1)
        assert body == "".join("%d %d\n" % l for l in links).encode()
        slots, keys, probe = (int(v) for v in last.split())
        want = n_key if cap < 0 else cap
        assert keys == n_key and slots & (slots - 1) == 0 and (slots >= 2 * n_key if not want else want <= slots < 2 * max(want, 1))
        assert probe <= slots
        probes.append(probe)
    return ug, links, probes


def test_model_on_the_hand_cases(program, tmp_path):
    kinds = set()
    for name, (k, seqs) in sorted(HAND.items()):
        x, c = table_of(seqs, k)
        for min_cnt in (1, 2):
            ug, links, _ = model_equals(program, tmp_path, name, k, x, c, min_cnt, caps=(0, -1))
            kinds.update(("cycle" if u[3] else "single" if u[1] == 1 else "chain") for u in ug)
            kinds.update("hairpin" for f, t in links if (t ^ 1, f ^ 1) == (f, t))
    assert kinds == {"cycle", "single", "chain", "hairpin"}
    x, c = table_of(HAND["polya"][1], 5)
    assert model_equals(program, tmp_path, "none", 5, x, c, 1023)[:2] == ([], [])      # a table without a node


def test_model_at_a_full_table(program, tmp_path):
    """512 unitigs of one node: 512 keys in 512 slots, no free slot left -- every claim and every look-up still ends, the longest after many slots"""
    k, seqs = HAND["every_5_mer"]
    x, c = table_of(seqs, k)
    ug, links, probes = model_equals(program, tmp_path, "full", k, x, c, 1, caps=(0, -1, 600))
    assert len(links) == 4096 and probes[0] < 32 < probes[1] and probes[2] <= probes[1]


def test_model_on_tiny_random_tables(program, tmp_path):
    rng = random.Random(5)
    n_link = 0
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        x, c = table_of(seqs, k)
        _, links, _ = model_equals(program, tmp_path, "t%d" % it, k, x, c, rng.choice((1, 1, 2)), caps=(0, -1))
        n_link += len(links)
    assert n_link > 1500


def test_model_on_reads_at_k31(program, oracle, synth, tmp_path):
    """reads with errors at k = 31: bubbles and tips by the hundred, more than 2048 oriented ends; the table in the listing order of a .yak file"""
    data, _ = oracle.count_protocol_mem(synth(2000, 150), k=31, pre=10, bf_shift=0)
    fn = str(tmp_path / "reads.yak")
    open(fn, "wb").write(data)
    k, x, c = U.members(fn)
    for min_cnt in (1, 3):
        ug, links, _ = model_equals(program, tmp_path, "reads", k, x, c, min_cnt, caps=(0, -1))
        if min_cnt == 1:
            assert len(ug) > 1024 and len(links) > 1000


def test_model_refuses(program, tmp_path):
    """a capacity below the number of keys, and descriptors that do not fit the bases: a message, not a walk without end or a read outside"""
    k, seqs = HAND["bubble"]
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, 1)
    ug = U.unitigs(k, recs, 1)
    amap, desc, bases = W.restate(k, recs, 1, ug)
    for name, cap, dd, bb, what in (("small", G.n_keys(ug) - 1, desc, bases, b"below the number of keys"),
                                    ("off", 0, [desc[0], (desc[1][0] + len(bases),) + desc[1][1:]] + desc[2:], bases, b"does not fit"),
                                    ("long", 0, desc[:-1] + [(desc[-1][0], desc[-1][1] + 1) + desc[-1][2:]], bases, b"does not fit"),
                                    ("huge", 0, [(desc[0][0], (1 << 64) - 2) + desc[0][2:]] + desc[1:], bases, b"does not fit"),
                                    ("nobase", 0, desc, bases[:3] + b"N" + bases[4:], b"does not fit")):
        fn = str(tmp_path / (name + ".gfm"))
        G.model_file(fn, k, 1, cap, st, ug, dd, bb)
        r = subprocess.run([program, fn, "gfa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and what in r.stderr, (name, r.stderr)
