"""The sequential model of the cleaning kernels (tests/tools/clean_model_check.cpp: the first link of every end, the clip rule, the pop rule, the count,
the scan, the emit and the image with the very functions of yak_amd/clean/clean_step.h, the report of clean_text.h; built with the host compiler under
the address and undefined-behaviour sanitizers and run as a program of its own, nothing of it is loaded into Python) against the restatement of
tests/clean_util.py, byte for byte, round by round: the report, the records and the image -- on the hand-derived cases of tests/test_clean.py, on tiny
random tables and on the planted reads; and its refusals on a damaged list of links, a damaged bubble record and a damaged descriptor."""
import os
import random
import shutil
import subprocess

import pytest

import bubble_util as B
import clean_util as K
import graph_util as U
import walk_util as W
from conftest import ROOT
from test_clean import CASES, PLANTED
from test_gfa import table_of


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++ on the path: the model of the kernels cannot be built"
    exe = str(tmp_path_factory.mktemp("clean") / "clean_model_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tools", "clean_model_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(program, fn, mode):
    r = subprocess.run([program, fn, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def parts(k, x, c, min_cnt, d):
    """the descriptors, the bases and the bubble rows of a restated round"""
    recs_g = U.graph(k, x, c, min_cnt)[0]
    amap, desc, bases = W.restate(k, recs_g, min_cnt, d["ug"])
    return desc, bases, B.as_rows(d["bubbles"])


def model_equals(program, tmp, name, k, seqs, min_cnt=1, T=None, P=100):
    """every round of the restated cleaning through the model; returns the rounds"""
    T = k if T is None else T
    x, c = table_of(seqs, k)
    tables = []
    done = K.rounds(k, x, c, min_cnt, T, P, step=lambda d, x_, c_: tables.append(keep(d, x_, c_)) or tables[-1])[0]
    if min_cnt > 1:
        x, c = x[c >= min_cnt], c[c >= min_cnt]
    for r, d in enumerate(done):
        xr, cr = (x, c) if r == 0 else tables[r - 1]
        desc, bases, bub = parts(k, xr, cr, min_cnt, d)
        fn = str(tmp / ("%s_c%d_r%d.clm" % (name, min_cnt, r)))
        K.model_file(fn, k, min_cnt, T, P, len(xr), desc, bases, d["links"], bub)
        assert run(program, fn, "report") == (K.head_line(k, min_cnt, T, P) + K.round_line(1, d["round"]) + K.list_lines(1, d["recs"])).encode()
        body, last = run(program, fn, "records").rsplit(b"S ", 1)
        assert body == "".join("%d %d %d %d %d %d\n" % row for row in K.as_rows(k, d["recs"])).encode()
        s = d["stats"]
        assert [int(v) for v in last.split()] == [s["n_tip"], s["tip_nodes"], s["n_tip_kept"], s["n_pop"], s["pop_nodes"], s["n_pop_kept"], len(d["recs"]), len(d["image"])]
        assert run(program, fn, "image") == d["image"]
    return done


def keep(d, x, c):
    import numpy as np
    m = np.array([int(v) not in d["gone"] for v in x], bool)
    return x[m], c[m]


def test_model_on_the_hand_cases(program, tmp_path):
    why, rounds = set(), set()
    for name, (seqs, P) in sorted(CASES.items()):
        for min_cnt in (1, 2):
            done = model_equals(program, tmp_path, name, 5, seqs, min_cnt, P=P)
            why.update(rec[1] for d in done for rec in d["recs"])
            rounds.add(len(done))
    assert why == {K.TIP, K.POP} and rounds == {1, 2, 3}
    for T, P in ((0, 100), (5, 0), (2, 100), (3, 1)):
        model_equals(program, tmp_path, "opt_%d_%d" % (T, P), 5, CASES["arm_forks"][0], T=T, P=P)
    assert model_equals(program, tmp_path, "none", 5, CASES["tip"][0], 1023)[0]["round"] == dict(n_key=0, n_unitig=0, n_link=0, n_bubble=0, n_tip=0, tip_nodes=0, n_pop=0,
                                                                                                pop_nodes=0, removed=0)


def test_model_on_tiny_random_tables(program, tmp_path):
    rng = random.Random(29)
    n_tip = n_pop = 0
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        if it % 2:                                               # a string of 20 to 30 bases and a copy with one base changed: bubbles
            k = 5
            a = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 30)))
            p = rng.randrange(6, len(a) - 6)
            seqs = [a, a[:p] + rng.choice([ch for ch in "ACGT" if ch != a[p]]) + a[p + 1:]]
        done = model_equals(program, tmp_path, "t%d" % it, k, seqs, rng.choice((1, 1, 2)), T=rng.choice((k, k, 2, 9)), P=rng.choice((100, 100, 50)))
        n_tip += sum(d["round"]["n_tip"] for d in done)
        n_pop += sum(d["round"]["n_pop"] for d in done)
    assert n_tip > 10 and n_pop > 0, (n_tip, n_pop)


def test_model_on_the_planted_reads(program, tmp_path):
    for k, seed in PLANTED:
        done = model_equals(program, tmp_path, "p%d" % k, k, K.planted_reads(k, seed)[1])
        assert [(d["round"]["n_tip"], d["round"]["n_pop"]) for d in done] == [(8, 12), (0, 0)]


def test_model_refuses(program, tmp_path):
    """a list of links that is not sorted by `from`, that leads to an end outside the unitigs, or that gives one end five links; a bubble record whose
    arm lies outside the unitigs; a removed unitig whose descriptor leaves the bases: a message, not a read outside"""
    k, seqs = 5, CASES["arm_forks"][0]
    x, c = table_of(seqs, k)
    first = K.one_round(k, x, c, 1, k, 100)
    x2, c2 = keep(first, x, c)
    for name, xr, cr in (("tips", x, c), ("pops", x2, c2)):
        d = K.one_round(k, xr, cr, 1, k, 100)
        desc, bases, bub = parts(k, xr, cr, 1, d)
        links, n_end, gone = d["links"], 2 * len(d["ug"]), d["recs"][0][0]
        f0 = links[0][0]
        cases = [("unsorted", [links[1], links[0]] + links[2:] if links[0][0] != links[1][0] else links[:1] + [links[2], links[1]] + links[3:], desc, bub, b"does not fit"),
                 ("to", links[:-1] + [(links[-1][0], n_end)], desc, bub, b"does not fit"),
                 ("from", links[:-1] + [(n_end + 3, links[-1][1])], desc, bub, b"does not fit"),
                 ("five", [(f0, t) for t in range(5)] + [l for l in links if l[0] > f0], desc, bub, b"does not fit"),
                 ("off", links, desc[:gone] + [(len(bases),) + desc[gone][1:]] + desc[gone + 1:], bub, b"does not lie inside the bases")]
        if bub:
            b0 = bub[0]
            cases.append(("arm", links, desc, [b0[:2] + (n_end, b0[3]) + b0[4:]] + bub[1:], b"a bubble record does not fit"))
            cases.append(("kc", links, desc, [b0[:6] + (b0[6] + 1,) + b0[7:]] + bub[1:], b"a bubble record does not fit"))
        for what, ll, dd, bb, msg in cases:
            fn = str(tmp_path / ("%s_%s.clm" % (name, what)))
            K.model_file(fn, k, 1, k, 100, len(xr), dd, bases, ll, bb)
            for mode in ("report", "records", "image"):
                r = subprocess.run([program, fn, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
                assert r.returncode == 1 and r.stdout == b"" and msg in r.stderr, (name, what, r.stderr)
