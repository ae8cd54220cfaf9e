"""The sequential model of the bubble kernels (tests/tools/bubble_model_check.cpp: the first link of every end, the count, the scan, the emit and the
classification with the very functions of yak_amd/bubble/bubble_step.h, the texts of bubble_text.h; built with the host compiler under the address
and undefined-behaviour sanitizers and run as a program of its own, nothing of it is loaded into Python) against the restatement of
tests/bubble_util.py, byte for byte: the B lines, the -s text and the records -- on the hand-derived cases of tests/test_bubble.py, on tiny random
tables and on the planted genomes; and its refusals on a damaged list of links."""
import os
import random
import shutil
import subprocess

import pytest

import bubble_util as B
import gfa_util as G
import graph_util as U
import walk_util as W
from conftest import ROOT
from test_bubble import HAND, PLANTED_SEEDS
from test_gfa import table_of


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++ on the path: the model of the kernels cannot be built"
    exe = str(tmp_path_factory.mktemp("bubble") / "bubble_model_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tools", "bubble_model_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(program, fn, mode):
    r = subprocess.run([program, fn, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def model_equals(program, d, name, k, seqs, min_cnt):
    """the three outputs of the model; returns (unitigs, records, stats)"""
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    amap, desc, bases = W.restate(k, recs, min_cnt, ug)
    links = G.links_by_strings(k, ug)
    want, bs = B.by_strings(k, ug)
    assert (want, bs) == B.by_links(k, ug, links)
    fn = str(d / ("%s_c%d.bbm" % (name, min_cnt)))
    B.model_file(fn, k, min_cnt, st, ug, desc, bases, links)
    assert run(program, fn, "text") == B.text(k, min_cnt, ug, want)
    assert run(program, fn, "stats") == B.stats_text(k, min_cnt, st, ug, links, bs)
    body, last = run(program, fn, "records").rsplit(b"T ", 1)
    assert body == "".join("%d %d %d %d %d %d %d %d %d %d\n" % r for r in B.as_rows(want)).encode()
    assert [int(v) for v in last.split()] == [bs["n_bubble"]] + bs["n_type"] + [bs["n_fork"], bs["n_tip"], bs["tip_nodes"], bs["max_arm_nodes"]]
    return ug, want, bs


def test_model_on_the_hand_cases(program, tmp_path):
    types, sides = set(), set()
    for name, (k, seqs) in sorted(HAND.items()):
        for min_cnt in (1, 2):
            ug, recs, bs = model_equals(program, tmp_path, name, k, seqs, min_cnt)
            types.update(r[6] for r in recs)
            sides.update(a & 1 for r in recs for a in r[2])
    assert types == set("SEI") and sides == {0, 1}
    assert model_equals(program, tmp_path, "none", 5, HAND["bubble"][1], 1023)[1:] == ([], dict(n_bubble=0, n_type=[0, 0, 0], n_tip=0, tip_nodes=0, max_arm_nodes=0, n_fork=0))


def test_model_on_tiny_random_tables(program, tmp_path):
    rng = random.Random(26)
    n_fork = n_bubble = 0
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        if it % 2:                                               # a string of 20 to 30 bases and a copy with one base changed: bubbles
            k = 5
            a = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 30)))
            p = rng.randrange(6, len(a) - 6)
            seqs = [a, a[:p] + rng.choice([ch for ch in "ACGT" if ch != a[p]]) + a[p + 1:]]
        bs = model_equals(program, tmp_path, "t%d" % it, k, seqs, rng.choice((1, 1, 2)))[2]
        n_fork += bs["n_fork"]
        n_bubble += bs["n_bubble"]
    assert n_fork > 300 and n_bubble > 0, (n_fork, n_bubble)


def test_model_on_the_planted_genomes(program, tmp_path):
    for (k, circular), seed in sorted(PLANTED_SEEDS.items()):
        seqs, want = B.planted(k, 1000, seed, circular)
        ug, recs, bs = model_equals(program, tmp_path, "p%d_%d" % (k, circular), k, seqs, 1)
        assert B.found(recs) == sorted(want)


def test_model_refuses(program, tmp_path):
    """a list of links that is not sorted by `from`, that leads to an end outside the unitigs, or that gives one end five links; an arm whose
    descriptor leaves the bases or whose bases are none of ACGT: a message, not a read outside"""
    k, seqs = HAND["two_snps"]
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, 1)
    ug = U.unitigs(k, recs, 1)
    amap, desc, bases = W.restate(k, recs, 1, ug)
    links = G.links_by_strings(k, ug)
    deg = G.end_deg(ug, links)
    n_end = 2 * len(ug)
    f0 = links[0][0]
    arm = B.by_links(k, ug, links)[0][0][2][0] >> 1
    at = desc[arm][0]
    cases = (("unsorted", [links[1], links[0]] + links[2:] if links[0][0] != links[1][0] else links[:1] + [links[2], links[1]] + links[3:], desc, bases, b"does not fit"),
             ("to", links[:-1] + [(links[-1][0], n_end)], desc, bases, b"does not fit"),
             ("from", links[:-1] + [(n_end + 3, links[-1][1])], desc, bases, b"does not fit"),
             ("five", [(f0, t) for t in range(5)] + [l for l in links if l[0] > f0], desc, bases, b"does not fit"),
             ("off", links, desc[:arm] + [(len(bases),) + desc[arm][1:]] + desc[arm + 1:], bases, b"an arm does not fit the bases"),
             ("nobase", links, desc, bases[:at + 6] + b"N" + bases[at + 7:], b"none of ACGT"))
    for name, ll, dd, bb, what in cases:
        fn = str(tmp_path / (name + ".bbm"))
        B.model_file(fn, k, 1, st, ug, dd, bb, ll, end_deg=deg)
        for mode in ("text", "records"):
            r = subprocess.run([program, fn, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            assert r.returncode == 1 and r.stdout == b"" and what in r.stderr, (name, r.stderr)
