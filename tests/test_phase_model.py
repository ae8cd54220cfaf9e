"""The sequential model of the kernels of the phasing (tools/phase_model_check.cpp: the compaction of the full records, the votes into the pair
table with its growth from 16 slots and at a capacity equal to twice its keys, the rounds of Boruvka's exactly as the kernels stage them, the
classification and the text, with the very functions of yak_amd/phase/phase_step.h and phase_text.h; built by tools/Makefile with the host compiler
under the address and undefined-behaviour sanitizers and run as a program of its own, nothing of it is loaded into Python) against the restatement
of tests/phase_util.py, byte for byte, in three chunk sizes, with the threads of every launch in either order -- on the hand-derived cases of
tests/test_phase.py, on tiny random vote tables, on reads through real bubbles and on a planted diploid; and its refusals on damaged input: a record's
bubble out of range, records out of seq order, a support list of the wrong length."""
import os
import random
import shutil
import subprocess

import pytest

import allele_util as A
import graph_util as U
import phase_util as PH
from conftest import ROOT
from test_allele import TWO, graph_of
from test_bubble import CIRCLE, HAND
from test_phase import HAND_TABLES, HET, HOM, planted, random_table


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++") is not None and shutil.which("make") is not None, "no g++ or no make on the path: the model of the kernels cannot be built"
    d = str(tmp_path_factory.mktemp("phase_model")) + os.sep
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "phase_model_check", "O=" + d], check=True, capture_output=True, text=True)
    return d + "phase_model_check"


def run(program, fn, mode, *more):
    r = subprocess.run([program, fn, mode] + [str(m) for m in more], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def split(obs, n_parts):
    """records of one numbering of sequences as n_parts chunks, cut where a sequence ends, each numbered from 0: (chunks, their heads)"""
    seqs = sorted({o[0] for o in obs})
    per = (len(seqs) + n_parts - 1) // n_parts if seqs else 1
    chunks, heads = [], []
    for p in range(n_parts):
        mine = seqs[p * per:(p + 1) * per]
        first = mine[0] if mine else 0
        chunks.append([(o[0] - first,) + tuple(o[1:]) for o in obs if mine and mine[0] <= o[0] <= mine[-1]])
        heads.append((len(mine), 0, 0, 0))
    return chunks, heads


def table_equals(program, tmp, name, n_bubble, sup, votes, rng, min_sup=2, min_link=2, parts=(1, 2, 5)):
    """the model on records made from a vote table against the restatement's text, in three cuts, both tables and both orders; the last file"""
    recs = PH.fake_recs(n_bubble)
    obs = PH.obs_of_votes(votes, rng)
    res = PH.kruskal(n_bubble, sup, votes, min_sup, min_link)
    n_vote = sum(c + t for c, t in votes.values())
    head = [len({o[0] for o in obs}), 0, 0, 0, len(obs), sum(1 for o in obs if o[2] & PH.FULL)]
    fn = None
    for n_parts in parts:
        chunks, heads = split(obs, n_parts)
        for edges, stats_only in ((1, 0), (0, 0), (1, 1)):
            fn = str(tmp / ("%s_%d_%d%d.bin" % (name, n_parts, edges, stats_only)))
            PH.model_file(fn, 15, 1, min_sup, min_link, edges, stats_only, recs, sup, chunks, heads)
            want = PH.text(15, 1, min_sup, min_link, edges, stats_only, recs, sup, head, votes, n_vote, res)
            for table, order in (("grow", "fwd"), ("tight", "rev")):
                assert run(program, fn, "text", table, order) == want, (name, n_parts, edges, stats_only, table, order)
    return fn


def reads_equal(program, tmp, name, k, ug, recs, reads, min_sup=2, min_link=2, chunk_sizes=(1 << 28, 1000, 1)):
    """the model on the observation records of reads against the restatement's text, which does not depend on the chunks"""
    want = None
    for chunk_size in chunk_sizes:
        w = PH.whole(k, ug, recs, reads, min_sup, min_link, chunk_size)
        text = PH.text(k, 1, min_sup, min_link, True, False, recs, w["sup"], w["head"], w["votes"], w["n_vote"], w["res"])
        assert want in (None, text)
        want = text
        parts = A.chunks(reads, chunk_size)
        heads = [(len(p), sum(len(reads[i]) for i in p), len(d["paths"]), len(d["steps"])) for p, d in zip(parts, w["per"])]
        fn = str(tmp / ("%s_%d.bin" % (name, chunk_size)))
        PH.model_file(fn, k, 1, min_sup, min_link, 1, 0, recs, w["sup"], [d["obs"] for d in w["per"]], heads)
        for table, order in (("grow", "fwd"), ("tight", "rev")):
            assert run(program, fn, "text", table, order) == want, (name, chunk_size, table, order)
    return fn, w


def test_model_on_the_hand_cases(program, tmp_path):
    rng = random.Random(1)
    for at, (n_bubble, votes, not_het) in enumerate(HAND_TABLES):
        sup = [HOM if b in not_het else HET for b in range(n_bubble)]
        for m, e in ((2, 2), (1, 1), (2, 3)):
            table_equals(program, tmp_path, "h%d" % at, n_bubble, sup, votes, rng, m, e)


def test_model_on_tiny_random_vote_tables(program, tmp_path):
    rng = random.Random(232)
    n_edge = n_disc = 0
    for it in range(25):
        n_bubble = rng.randint(2, 12)
        sup, votes = random_table(rng, n_bubble)
        m, e = rng.choice((1, 2, 3)), rng.choice((1, 2))
        table_equals(program, tmp_path, "t%d" % it, n_bubble, sup, votes, rng, m, e, parts=(1, 3))
        res = PH.kruskal(n_bubble, sup, votes, m, e)
        n_edge += res["stats"]["n_edge"]; n_disc += res["stats"]["n_disc"]
    assert n_edge >= 40 and n_disc >= 2, (n_edge, n_disc)


def test_model_grows_its_table_and_holds_it_tight(program, tmp_path):
    """a complete graph on 24 bubbles, 276 pairs fed in forty chunks: the table grows from 16 slots more than once, and at 1024 slots it stands at
    the capacity of its keys from the first vote; long chains with rising and with equal weights need their rounds"""
    rng = random.Random(5)
    n = 24
    votes = {(i, j): [rng.randint(0, 5), rng.randint(1, 5)] for i in range(n) for j in range(i + 1, n)}
    fn = table_equals(program, tmp_path, "full", n, [HET] * n, votes, rng, 2, 1, parts=(40,))
    n_pair = len(votes)
    g = run(program, fn, "table", "grow").split()
    assert g[0] == b"G" and int(g[1]) >= 2 and int(g[2]) >= 2 * n_pair and int(g[3]) == n_pair
    t = run(program, fn, "table", "tight").split()
    assert (int(t[1]), int(t[2]), int(t[3])) == (0, 1024, n_pair) and 512 < 2 * n_pair <= 1024
    for name, weight in (("rise", lambda i: i + 1), ("equal", lambda i: 3)):
        m = 200
        votes = {(i, i + 1): ([weight(i), 0] if i % 3 else [0, weight(i)]) for i in range(m - 1)}
        fn = table_equals(program, tmp_path, name, m, [HET] * m, votes, rng, 2, 1, parts=(2,))
        rounds = int(run(program, fn, "table", "grow").split()[4])
        assert 2 <= rounds <= 9, (name, rounds)                    # at most ceil(log2 200) + 1


def test_model_on_reads_through_real_bubbles(program, tmp_path):
    ug, recs = graph_of(TWO, 5)
    reads = [r.encode() for r in (TWO[0], TWO[1], U.rc_str(TWO[0][:14] + TWO[1][14:]), TWO[0][:15], TWO[1][12:], TWO[0], TWO[1])]
    reads_equal(program, tmp_path, "two", 5, ug, recs, reads, chunk_sizes=(1 << 28, 40, 1))
    k, seqs = HAND["circle"]
    ug, recs = graph_of(seqs, k)
    read = CIRCLE * 2 + CIRCLE[:8]
    reads_equal(program, tmp_path, "circle", k, ug, recs, [read.encode(), U.rc_str(read).encode()], min_sup=1, chunk_sizes=(1 << 28, 1))


def test_model_on_a_planted_diploid(program, tmp_path):
    a, b, pos, behind, ug, recs, reads = planted(1)
    fn, w = reads_equal(program, tmp_path, "dip", 15, ug, recs, reads, chunk_sizes=(1 << 28, 5000, 1))
    assert w["res"]["stats"]["n_block"] == 2 and w["n_vote"] > 300 and int(run(program, fn, "table", "grow").split()[1]) >= 1


def test_model_refuses_damaged_input(program, tmp_path):
    """a record's bubble out of range, records out of seq order, a support list one entry short: a message, no text, and never a read outside"""
    rng = random.Random(9)
    fn = table_equals(program, tmp_path, "ok", 4, [HET] * 4, {(0, 1): [0, 4], (1, 2): [3, 0], (2, 3): [0, 2]}, rng, parts=(1,))
    for mode, what in (("damage-bubble", b"records do not fit"), ("damage-order", b"records do not fit"), ("damage-sup", b"the support is not that of the bubbles")):
        for table, order in (("grow", "fwd"), ("tight", "rev")):
            r = subprocess.run([program, fn, mode, table, order], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
            assert r.returncode == 1 and r.stdout == b"" and what in r.stderr, (mode, r.stderr)
    r = subprocess.run([program, str(tmp_path / "none.bin"), "text"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and b"cannot read the file" in r.stderr
