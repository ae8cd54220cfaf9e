"""`yak-amd cover`, its definition restated twice in tests/cover_util.py -- flat numpy over the per-position count array, and
by strings with a dict and itertools.groupby -- held to each other on the oracle's lookups of synthetic reads (with N, lower case and sequences
shorter than k), to the reference's own `qv -p` numbers, and to cases derived by hand."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD
import cover_util as U
from test_depth import oracle_counts
from test_qv import query_file

QV = json.load(open(os.path.join(GOLD, "qv.json")))
NO = U.NOKMER


@pytest.mark.parametrize("k", [21, 31, 5])
def test_the_two_restatements_agree(k, oracle, synth):
    O = oracle.lib()
    reads = synth(400, 150, 2500, s=5)
    opt = oracle.copt(k, 10, 4, 0, 10000000)
    o = O.yko_count_protocol_mem(reads, len(reads), None, 0, C.byref(opt))
    assert o
    try:
        recs = U.variants(synth(12, 300, 2500, s=5, e=0.02, N=0.0).split(b"\n")[:-1], k)
        seqs = [s for _, s in recs]
        img, offs, lens = U.image(seqs)
        t = oracle.lookup_image(o, img, 2)
        count_of = U.count_dict(oracle, o, seqs, k)
    finally:
        O.yko_ch_destroy(o)
    assert any(b"N" in s for s in seqs) and any(s != s.upper() for s in seqs) and min(len(s) for s in seqs) == 1
    for lo, hi in ((1, 1023), (0, 0), (2, 5), (1023, 1023)):
        a_t, a_i = U.tallies(t, offs, lens, k, lo, hi), U.intervals(t, offs, lens, k, lo, hi)
        b = U.by_strings(seqs, count_of, k, lo, hi)
        assert [tuple(int(v) for v in x) for x in a_t] == [r[:4] for r in b], (lo, hi)
        assert a_i == [r[4] for r in b], (lo, hi)
        assert [len(r) for r in a_i] == a_t["n_run"].tolist()
    if k == 21:                                             # the planted stretch is what 0:0 finds, and 1:1023 leaves out
        j = [n for n, _ in recs].index(b"planted")
        assert any(st <= 45 and en >= 105 for st, en in U.intervals(t, offs, lens, k, 0, 0)[j])
        assert all(en <= 45 + k or st >= 105 - k for st, en in U.intervals(t, offs, lens, k, 1, 1023)[j])
        sep = np.asarray(offs[1:], np.int64) - 1
        assert not U.cov(t, k, 0, 1023)[sep].any()          # a separator is never covered, whatever the predicate


@pytest.mark.parametrize("name", sorted(QV))
def test_restatement_has_the_reference_numbers(name, oracle, tmp_path):
    """lo = 1, hi = 1023: n_kmer and n_hit per sequence are the tot and non0 of the reference's `qv -p` SQ lines"""
    desc = QV[name]
    O = oracle.lib()
    o = O.yko_ch_restore(os.path.join(GOLD, desc["table"] + ".yak").encode())
    assert o
    try:
        k = o.contents.k
        recs = U.read_fastx(query_file(desc, tmp_path))
        img, offs, lens = U.image([s for _, s in recs])
        t = oracle_counts(oracle, o, img, k)
    finally:
        O.yko_ch_destroy(o)
    sq = {f[1]: (int(f[2]), int(f[3]), int(f[4])) for f in (ln.split("\t") for ln in desc["sq"])}
    assert len(sq) > 0
    tl = U.tallies(t, offs, lens, k, 1, 1023)
    seen = 0
    for (nm, seq), x in zip(recs, tl):
        if nm.decode() in sq:
            assert (len(seq), int(x["n_kmer"]), int(x["n_hit"])) == sq[nm.decode()], nm
            seen += 1
    assert seen == len(sq)


# ---- by hand ----
def one(t, k, lo, hi, L=None):
    t = np.array(t, np.uint16)
    L = len(t) if L is None else L
    x = U.tallies(t, [0], [L], k, lo, hi)[0]
    return U.cov(t, k, lo, hi).tolist(), tuple(int(v) for v in x), U.intervals(t, [0], [L], k, lo, hi)[0]


def test_k3_by_hand():
    t = [NO, NO, 5, 0, NO, 7]
    # 1:1023 -- hits at 2 and 5: the k-mer ending at 2 covers 0..2, the one ending at 5 covers 3..5
    assert one(t, 3, 1, 1023) == ([1, 1, 1, 1, 1, 1], (3, 2, 6, 1), [(0, 6)])
    # 0:0 -- the hit is element 3: bases 1..3
    assert one(t, 3, 0, 0) == ([0, 1, 1, 1, 0, 0], (3, 1, 3, 1), [(1, 4)])
    # 5:5 -- the hit is element 2: bases 0..2
    assert one(t, 3, 5, 5) == ([1, 1, 1, 0, 0, 0], (3, 1, 3, 1), [(0, 3)])


def test_single_hit_at_the_last_position():
    assert one([NO, NO, 0, 0, 0, 9], 3, 1, 1023) == ([0, 0, 0, 1, 1, 1], (4, 1, 3, 1), [(3, 6)])
    assert one([9], 1, 1, 1023) == ([1], (1, 1, 1, 1), [(0, 1)])
    assert one([0] * 14 + [3], 21, 1, 1023) == ([1] * 15, (15, 1, 15, 1), [(0, 15)])       # an array shorter than k
    assert one([4000, NO], 3, 1000, 1023) == ([1, 0], (1, 1, 1, 1), [(0, 1)])      # above 1023 reads as 1023; the cover ends with the array


def test_hits_k_apart_and_k_minus_1_apart():
    """`apart` = the positions between the two ends: with k of them one base stays uncovered, with k - 1 the two k-mers touch"""
    k = 4
    t = [0] * 16
    t[5] = t[10] = 7                                        # k positions between (6..9): bases 2..5 and 7..10, base 6 is left out -- two runs
    assert one(t, k, 1, 1023)[1:] == ((16, 2, 8, 2), [(2, 6), (7, 11)])
    t = [0] * 16
    t[5] = t[9] = 7                                         # k - 1 between: bases 2..5 and 6..9 touch -- one run of 8
    assert one(t, k, 1, 1023)[1:] == ((16, 2, 8, 1), [(2, 10)])
    t = [0] * 16
    t[5] = t[8] = 7                                         # closer still: they overlap in one base -- one run of 7
    assert one(t, k, 1, 1023)[1:] == ((16, 2, 7, 1), [(2, 9)])
    assert one([NO, NO, 3, NO, NO, NO, 3], 3, 1, 1023)[1:] == ((2, 2, 6, 2), [(0, 3), (4, 7)])      # k = 3, three positions between


def test_runs_are_counted_per_sequence():
    """a run that goes on across two adjacent sequences of a hand-built array starts anew at off[s]"""
    t = np.array([1, 1, 1, 1, 0, 0], np.uint16)
    x = U.tallies(t, [0, 2], [2, 4], 1, 1, 1023)
    assert [tuple(int(v) for v in r) for r in x] == [(2, 2, 2, 1), (4, 2, 2, 1)]
    assert U.intervals(t, [0, 2], [2, 4], 1, 1, 1023) == [[(0, 2)], [(0, 2)]]


def test_masks():
    img = b"AC\x02gN-Tz@[\n"
    c = np.ones(len(img), np.uint8)
    assert U.masked(img, c, 0) == img
    assert U.masked(img, c, 1) == b"ac\x02gn-tz@[\n"       # letters alone; the raw base 2 and the bytes next to the letters' range stay
    assert U.masked(img, c, 2) == b"N" * len(img)
    c[::2] = 0
    assert U.masked(img, c, 1) == b"Ac\x02gN-Tz@[\n" and U.masked(img, c, 2) == b"AN\x02NNNTN@N\n"
    assert U.masked(bytes(range(256)), np.ones(256, np.uint8), 1) == bytes(b | 0x20 if chr(b).isalpha() and b < 128 else b for b in range(256))


def test_selection_at_an_exact_tie():
    # n_cov == min_frac * len: 3 of 6 at 0.5 is selected, and -v turns it round
    assert U.selected(1, 3, 6, min_frac=0.5) and not U.selected(1, 3, 6, min_frac=0.5, invert=True)
    assert not U.selected(1, 2, 6, min_frac=0.5) and U.selected(1, 2, 6, min_frac=0.5, invert=True)
    assert U.selected(2, 0, 6, min_hit=2) and not U.selected(1, 6, 6, min_hit=2)
    assert U.selected(0, 0, 0) and U.selected(0, 0, 0, min_frac=1.0) and not U.selected(0, 0, 0, invert=True)


def test_text_and_fasta_builders():
    k = 3
    img = b"ACGTAC\nGGN\n\n"
    offs, lens = [0, 7, 11], [6, 3, 0]
    t = np.array([NO, NO, 5, 0, NO, 7, NO, NO, NO, NO, NO, NO], np.uint16)
    names = [b"a", b"b", b"e"]
    assert U.text(names, t, offs, lens, k) == b"#cover\tk=3\tlo=1\thi=1023\nS\ta\t6\t3\t2\t6\t1\nS\tb\t3\t0\t0\t0\t0\nS\te\t0\t0\t0\t0\t0\nT\t3\t3\t9\t3\t2\t6\n"
    assert U.text(names, t, offs, lens, k, 0, 0, intervals_too=True, min_hit=1) == b"#cover\tk=3\tlo=0\thi=0\nS\ta\t6\t3\t1\t3\t1\nB\ta\t1\t4\nT\t3\t1\t9\t3\t1\t3\n"
    assert U.text(names, t, offs, lens, k, 0, 0, min_frac=0.5, invert=True) == b"#cover\tk=3\tlo=0\thi=0\nS\tb\t3\t0\t0\t0\t0\nT\t3\t1\t9\t3\t1\t3\n"
    assert U.fasta(names, img, t, offs, lens, k, 0, 0, mask=1) == b">a\nAcgtAC\n>b\nGGN\n>e\n\n"
    assert U.fasta(names, img, t, offs, lens, k, 0, 0, mask=2, min_frac=0.5) == b">a\nANNNAC\n>e\n\n"
    assert U.fasta(names, img, t, offs, lens, k, 0, 0, mask=0, min_frac=0.5, invert=True) == b">b\nGGN\n"
    assert U.by_strings([b"ACGTAC"], {b"ACG": 5, b"CGT": 0, b"GTA": 2, b"TAC": 7}, 3, 0, 0) == [(4, 1, 3, 1, [(1, 4)])]
