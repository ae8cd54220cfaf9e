"""`yak-amd depth`, its definition restated in numpy (tests/depth_util.py), held to the reference's own numbers: on the
per-position counts the oracle gives (yko_ch_get per k-mer) for the query and table of every case of tests/golden/qv.json, the whole-sequence
windows have the reference's total and present k-mers (its SQ lines), and the values of all windows of the sequences `yak qv` kept are the
reference's count histogram -- whatever the window.  Then the edges of the definition by hand."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD
import depth_util as U
from test_qv import query_file

QV = json.load(open(os.path.join(GOLD, "qv.json")))
NO = U.NOKMER


def oracle_counts(oracle, o, img, k):
    """max(0, yko_ch_get()) of the k-mer ending at every position of img, 0xffff where none ends"""
    O = oracle.lib()
    hh, tt = np.empty(len(img), np.uint64), np.empty(len(img), np.uint32)
    m = O.yko_extract_pos(k, img, len(img), hh.ctypes.data, tt.ctypes.data)
    t = np.full(len(img), NO, np.uint16)
    for j in range(m):
        t[tt[j]] = max(0, O.yko_ch_get(o, int(hh[j])))
    assert np.array_equal(t, oracle.lookup_image(o, img, 2))
    return t


@pytest.mark.parametrize("name", sorted(QV))
def test_restatement_has_the_reference_numbers(name, oracle, tmp_path):
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
    args = desc["args"]
    min_len = int(args[args.index("-l") + 1]) if "-l" in args else 0
    min_frac = float(args[args.index("-f") + 1]) if "-f" in args else 0.5
    whole = U.depth(t, offs, lens, k, 0)
    sq = {f[1]: (int(f[2]), int(f[3]), int(f[4])) for f in (ln.split("\t") for ln in desc["sq"])}
    assert len(sq) > 0
    kept = []
    for j, ((nm, seq), (w0,)) in enumerate(zip(recs, whole)):
        if nm.decode() in sq:
            assert (len(seq), w0[2], w0[3]) == sq[nm.decode()], nm
        if len(seq) >= min_len and not (w0[3] < w0[2] * min_frac):                 # qv.c:45 and qv.c:83
            kept.append(j)
    assert kept
    want = {int(c): n for c, n in desc["cnt"].items()}
    for w in (0, 1, 97, 1000):
        hist = np.zeros(1024, np.int64)
        n_kmer = 0
        for j in kept:
            rows = U.depth(t, offs[j:j + 1], lens[j:j + 1], k, w)[0]
            assert [r[:2] for r in rows] == U.windows(int(lens[j]), w)
            for st, en in U.windows(int(lens[j]), w):
                hist += np.bincount(U.window_values(t, int(offs[j]), int(lens[j]), k, st, en), minlength=1024)
            n_kmer += sum(r[2] for r in rows)
            assert sum(r[4] for r in rows) == whole[j][0][4] and max(r[6] for r in rows) == whole[j][0][6]
        assert {c: int(n) for c, n in enumerate(hist) if n} == want, w
        assert n_kmer == hist.sum()


# ---- the definition's edges by hand: k = 3, so a sequence of L positions has its k-mers at elements 2 .. L - 1 ----
def one(vals, k=3, w=0, lead=NO):
    """the windows of one sequence whose k-mer counts are vals (its first k - 1 elements hold `lead`)"""
    t = np.array([lead] * (k - 1) + list(vals) + [NO], np.uint16)
    return [r[2:] for r in U.depth(t, [0], [len(t) - 1], k, w)[0]], U.text([b"s"], t, [0], [len(t) - 1], k, w)


def test_lower_median_even_and_odd():
    assert one([5, 1, 9])[0] == [(3, 3, 15, 5, 9)]
    assert one([5, 1, 9, 7])[0] == [(4, 4, 22, 5, 9)]                  # sorted 1 5 7 9: index (4 - 1) / 2 = 1
    assert one([4])[0] == [(1, 1, 4, 4, 4)]
    assert one([4, 2])[0] == [(2, 2, 6, 2, 4)]


def test_ties_all_equal_and_the_extremes():
    assert one([2, 7, 7, 7, 9, 1])[0] == [(6, 6, 33, 7, 9)]             # 1 2 7 7 7 9: index 2
    assert one([7, 7, 1, 7, 9, 9, 9, 7])[0] == [(8, 8, 56, 7, 9)]       # 1 7 7 7 7 9 9 9: index 3, the tie spans the middle
    assert one([6] * 10)[0] == [(10, 10, 60, 6, 6)]
    assert one([0, 1023, 0, 1023])[0] == [(4, 2, 2046, 0, 1023)]
    assert one([0, 1023, 1023])[0] == [(3, 2, 2046, 1023, 1023)]
    assert one([0, 0, 0])[0] == [(3, 0, 0, 0, 0)]


def test_no_kmer_windows():
    rows, txt = one([NO, NO, NO, NO])                                   # only N
    assert rows == [(0, 0, 0, 0, 0)] and txt == U.HEADER + b"s\t0\t6\t0\t0\t0.000\t0\t0\n"
    assert one([NO, 3, NO, 8, NO])[0] == [(2, 2, 11, 3, 8)]             # absent positions are skipped, not counted as 0
    t = np.array([9, NO], np.uint16)                                    # L = 1 < k: the lead-in value belongs to no window
    assert U.depth(t, [0], [1], 3, 0) == [[(0, 1, 0, 0, 0, 0, 0)]]
    assert U.depth(t, [0], [1], 3, 1) == [[(0, 1, 0, 0, 0, 0, 0)]]
    assert U.depth(np.array([NO], np.uint16), [0], [0], 3, 0) == [[(0, 0, 0, 0, 0, 0, 0)]]      # an empty sequence has one window
    assert U.depth(np.array([NO], np.uint16), [0], [0], 3, 5) == [[(0, 0, 0, 0, 0, 0, 0)]]
    assert list(U.win_off([0, 1, 5, 6], 5)) == [0, 1, 2, 3, 5] and list(U.win_off([0, 9], 0)) == [0, 1, 2]


def test_window_cutting():
    vals = [1, 2, 3, 4, 5, 6, 7]                                        # L = 9, k = 3: starts 0 .. 6 have a k-mer
    rows, txt = one(vals, w=1, lead=500)
    assert rows == [(1, 1, v, v, v) for v in vals] + [(0, 0, 0, 0, 0)] * 2      # starts 7 and 8: windows without a k-mer
    assert txt.split(b"\n")[1] == b"s\t0\t1\t1\t1\t1.000\t1\t1" and txt.split(b"\n")[9] == b"s\t8\t9\t0\t0\t0.000\t0\t0"
    assert one(vals, w=4, lead=500)[0] == [(4, 4, 10, 2, 4), (3, 3, 18, 6, 7), (0, 0, 0, 0, 0)]   # w does not divide L; the last window holds starts >= L - k + 1 only
    assert one(vals, w=7, lead=500)[0] == [(7, 7, 28, 4, 7), (0, 0, 0, 0, 0)]
    assert one(vals, w=9, lead=500)[0] == one(vals, w=0, lead=500)[0] == one(vals, w=100, lead=500)[0] == [(7, 7, 28, 4, 7)]
    assert one(vals, w=3)[1] == U.HEADER + b"s\t0\t3\t3\t3\t2.000\t2\t3\ns\t3\t6\t3\t3\t5.000\t5\t6\ns\t6\t9\t1\t1\t7.000\t7\t7\n"
    assert one([1, 2, 2], w=0)[1] == U.HEADER + b"s\t0\t5\t3\t3\t1.667\t2\t2\n"


def test_neighbours_do_not_leak():
    """two sequences side by side: the separator, and the k - 1 lead-in elements of the second, hold counts that belong to no window"""
    k = 3
    t = np.array([800, 800, 1, 2, 900, 800, 800, 5, 900], np.uint16)    # s0 = elements 0..3, separator, s1 = elements 5..7, separator
    assert U.depth(t, [0, 5], [4, 3], k, 0) == [[(0, 4, 2, 2, 3, 1, 2)], [(0, 3, 1, 1, 5, 5, 5)]]
    assert U.depth(t, [0, 5], [4, 3], k, 2) == [[(0, 2, 2, 2, 3, 1, 2), (2, 4, 0, 0, 0, 0, 0)], [(0, 2, 1, 1, 5, 5, 5), (2, 3, 0, 0, 0, 0, 0)]]
    s = U.structs(t, [0, 5], [4, 3], k, 2)
    assert s.dtype.itemsize == 24 and s["sum"].tolist() == [3, 0, 5, 0] and s["median"].tolist() == [1, 0, 5, 0]
