"""`yak-amd correct` on the device (yak_amd/correct/correct.hip behind the four device-level calls of include/yak_amd_correct.h, yakamd_correct, the
CLI and yak_amd.correct) against the restatement of tests/correct_util.py (held to a second restatement and to hand-derived cases by
tests/test_correct.py): the find record by record and tally by tally on count arrays built around every edge of the kernel's tiling, the trial
image byte by byte, the decisions field by field with the corrected image, yakamd_correct_image_dev against the three calls on the dump of the
very table looked up, 4 KiB behind every output, the launches of an empty image and of one without candidates, the command byte for byte in three
chunk sizes from FASTA, FASTQ and gzip, the planted reads restored, idempotence, n_weak_after against a lookup of the output, and the refusals."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import correct_util as K
import paths_util as PU
from conftest import ROOT
from test_correct import CASES, G, HAND_TABLE, KERNELS, PLANTED, mut

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
TILE = 1024                                    # positions per tile of k_cor_find
GROUP = 8                                      # tiles per workgroup: the scan runs over the groups' sums
PAD = 4096                                     # bytes behind every output buffer that must stay as they were
FILL = 0xA5
SOLID = 7


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def co(ya):
    import yak_amd.correct as correct
    correct.lib()
    return correct


class Dev:
    def __init__(self, L):
        self.L, self.bufs = L, []

    def put(self, arr, pad=0):
        data = np.ascontiguousarray(arr).tobytes() + bytes([FILL]) * pad
        p = self.L.yakamd_dev_alloc(max(len(data), 16))
        assert p
        self.bufs.append(p)
        if data:
            assert self.L.yakamd_memcpy_h2d(p, data, len(data)) == 0
        return p

    def get(self, p, n):
        raw = np.empty(n, np.uint8)
        if n:
            assert self.L.yakamd_memcpy_d2h(raw.ctypes.data, p, n) == 0
        return raw

    def free(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)
        self.bufs = []


@pytest.fixture()
def dev(ya):
    d = Dev(ya.lib())
    yield d
    d.free()


def padded(a, dtype, fill):
    """the array in room for a multiple of 16 elements"""
    out = np.full(K.up16(len(a)), fill, dtype)
    out[:len(a)] = a
    return out


def find_dev(co, dev, t, offs, lens, k, c, e, cap=None, with_tally=True):
    """yakamd_correct_find_dev on the count array -> (its return value, the records, the tallies); every output is pre-filled and checked behind
    its end.  cap None: the counting call first, then the list of exactly that size"""
    CL = co.lib()
    n, ns = len(t), len(lens)
    d_t, d_off, d_len = dev.put(padded(t, np.uint16, SOLID)), dev.put(np.asarray(offs, np.uint64)), dev.put(np.asarray(lens, np.uint32))
    d_tal = dev.put(np.full(ns * 32, FILL, np.uint8), PAD) if with_tally else None
    if cap is None:
        cap = CL.yakamd_correct_find_dev(k, c, e, d_t, n, d_off, d_len, ns, None, 0, d_tal)
        assert cap >= 0, co._err()
    d_fix = dev.put(np.full(cap * 32, FILL, np.uint8), PAD)
    r = CL.yakamd_correct_find_dev(k, c, e, d_t, n, d_off, d_len, ns, d_fix, cap, d_tal)
    assert r >= 0, co._err()
    fix = dev.get(d_fix, cap * 32 + PAD)
    assert (fix[cap * 32:] == FILL).all(), "written behind the records"
    tal = None
    if with_tally:
        tal = dev.get(d_tal, ns * 32 + PAD)
        assert (tal[ns * 32:] == FILL).all(), "written behind the tallies"
        tal = tal[:ns * 32].view(K.TALLY_DTYPE)
    return r, fix[:cap * 32], tal


def check_find(co, dev, t, offs, lens, k, c, e):
    want, wtal = K.find(t, offs, lens, k, c, e)
    r, fix, tal = find_dev(co, dev, t, offs, lens, k, c, e)
    assert r == len(want)
    got = fix.view(K.FIX_DTYPE)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (k, c, e, bad[:4], got[bad[:4]], want[bad[:4]])
    bad = np.flatnonzero(tal != wtal)
    assert bad.size == 0, (k, c, e, bad[:4], tal[bad[:4]], wtal[bad[:4]])
    return want, wtal


def edge_blocks(k):
    """a count array of blocks of two tiles, a sequence each: a run that starts or ends at every offset around the tile edge inside the block and
    around the end of the halo behind it, of 1, 2, k - 1, k, k + 1 and k + 2 positions, with both neighbours solid, with none in front, with none
    behind and with neither"""
    blocks = []
    for L in sorted({1, 2, k - 1, k, k + 1, k + 2}):
        for kind in ("mid", "front", "back", "alone"):
            for delta in list(range(-(k + 3), 3)):
                for anchor in ("start", "end"):
                    st = TILE + delta if anchor == "start" else TILE + delta - L
                    blocks.append((st, st + L, kind))
    n = 2 * TILE * len(blocks)
    t = np.full(n, K.NO, np.uint16)
    offs, lens = [], []
    for b, (st, en, kind) in enumerate(blocks):
        o, L = 2 * TILE * b + 3, 2 * TILE - 8                      # the sequence: bytes [o, o + L), a k-mer from o + k - 1 on
        offs.append(o); lens.append(L)
        lo = o + k - 1 if kind in ("mid", "back") else 2 * TILE * b + st
        hi = o + L if kind in ("mid", "front") else 2 * TILE * b + en
        t[lo:hi] = SOLID
        t[2 * TILE * b + st:2 * TILE * b + en] = b % 3               # weak under min_cnt 3, absent or present
    return t, np.array(offs, np.uint64), np.array(lens, np.uint32)


# ---- the find ----
@pytest.mark.parametrize("k", [5, 21, 31])
def test_find_around_every_tile_edge(co, dev, k):
    """at k 21 and 31 more groups of tiles than the scan has threads as well: a few hundred of them"""
    t, offs, lens = edge_blocks(k)
    assert len(t) // (GROUP * TILE) > 256 or k == 5
    for e in (1, 3):
        want, wtal = check_find(co, dev, t, offs, lens, k, 3, e)
        L = want["en"].astype(int) - want["st"].astype(int)
        assert set(L) == {v for v in (1, 2, k - 1, k) if v >= e} and (want["p"] < want["st"]).any() and ((want["p"] == want["st"]) & (L < k)).any()
        dev.free()
    check_find(co, dev, t, offs, lens, k, 1, 1)                  # min_cnt 1: only the absent ones are weak


def test_find_runs_of_k_and_k_plus_1_straddle_two_tiles(co, dev):
    k = 21
    t = np.full(4 * TILE, SOLID, np.uint16)
    t[:k - 1] = K.NO
    t[4 * TILE - 1] = K.NO
    t[TILE - 10:TILE - 10 + k] = 0                               # k positions over the first edge: a candidate
    t[2 * TILE - 10:2 * TILE - 10 + k + 1] = 1                   # k + 1 over the second: none
    t[3 * TILE - 1:3 * TILE + 1] = 2                             # two over the third with both neighbours solid: none
    want, wtal = check_find(co, dev, t, [0], [4 * TILE - 1], k, 3, 1)
    assert [(int(r["p"]), int(r["st"]), int(r["en"])) for r in want] == [(TILE - 10, TILE - 10, TILE + 11)]
    assert tuple(wtal[0])[:3] == (4 * TILE - k, 2 * k + 3, 1)


def test_find_sizes_and_the_counting_call(co, dev):
    """arrays of 1, 15, 16, 17 positions and around a tile; the counting call and a call with too small a list write no record"""
    rng = np.random.default_rng(30)
    k = 5
    for n in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 77):
        t = np.where(rng.random(n) < 0.1, 0, SOLID).astype(np.uint16)
        t[rng.random(n) < 0.03] = K.NO
        t[:min(k - 1, n)] = K.NO
        check_find(co, dev, t, [0], [n], k, 3, 1)
        dev.free()
    t = np.full(300, SOLID, np.uint16)
    t[:4] = K.NO
    t[50:55] = t[100:105] = t[200:205] = 0
    want, wtal = K.find(t, [0], [300], k, 3, 1)
    assert len(want) == 3
    for cap in (0, 2):
        r, fix, tal = find_dev(co, dev, t, [0], [300], k, 3, 1, cap=cap)
        assert r == 3 and (fix == FILL).all() and (tal == wtal).all()
    r, fix, tal = find_dev(co, dev, t, [0], [300], k, 3, 1, cap=5, with_tally=False)      # room to spare, no tallies
    assert r == 3 and (fix[:96].view(K.FIX_DTYPE) == want).all() and (fix[96:] == FILL).all()
    # sequences that are empty, that leave bytes between them, and a run in no sequence
    t = np.full(400, SOLID, np.uint16)
    t[:4] = K.NO
    t[[99, 100, 101, 102, 103, 250]] = K.NO
    t[40:45] = t[104:106] = t[300:305] = 0
    offs, lens = [0, 99, 100, 100, 260], [99, 0, 0, 150, 20]
    want, wtal = check_find(co, dev, t, offs, lens, k, 3, 1)
    assert [(int(r["seq"]), int(r["p"])) for r in want] == [(0, 40), (3, 1)]
    # more sequences in a tile than the kernel keeps in LDS (96): 400 reads of 8 bases, then reads of 150, so that both ways are taken
    lens = np.array([8] * 400 + [150] * 40, np.uint32)
    offs = np.concatenate(([0], np.cumsum(lens[:-1].astype(np.uint64) + 1))).astype(np.uint64)
    n = int(offs[-1]) + int(lens[-1]) + 1
    t = np.where(rng.random(n) < 0.3, 0, SOLID).astype(np.uint16)
    for o, L in zip(offs, lens):
        t[int(o):int(o) + k - 1] = K.NO
        t[int(o) + int(L)] = K.NO
    want, wtal = check_find(co, dev, t, offs, lens, k, 3, 1)
    assert len(want) > 250 and TILE // 9 > 96 and (wtal["n_cand"][:400] > 0).sum() > 100 and (wtal["n_cand"][400:] > 0).sum() > 10


# ---- the trial image and the decisions ----
def trials_dev(co, dev, img, recs, k, want_rc=None):
    CL = co.lib()
    n, nf = len(img), len(recs)
    d_img, d_fix = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10)), dev.put(recs)
    need = CL.yakamd_correct_trials_dev(k, d_img, n, d_fix, nf, None, 0)
    assert need == K.up16(6 * k * nf)
    d_tr = dev.put(np.full(need, FILL, np.uint8), PAD)
    assert CL.yakamd_correct_trials_dev(k, d_img, n, d_fix, nf, d_tr, need - 1) == need and (dev.get(d_tr, need + PAD) == FILL).all()
    r = CL.yakamd_correct_trials_dev(k, d_img, n, d_fix, nf, d_tr, need)
    if want_rc is not None:
        assert r == want_rc
        return None
    assert r == need, co._err()
    out = dev.get(d_tr, need + PAD)
    assert (out[need:] == FILL).all(), "written behind the trial image"
    return out[:need].tobytes()


def decide_dev(co, dev, img, recs0, tal0, tc, k, c):
    CL = co.lib()
    n, nf, ns = len(img), len(recs0), len(tal0)
    room = K.up16(n)
    d_img = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10), PAD)
    d_fix, d_tal, d_tc = dev.put(recs0, PAD), dev.put(tal0, PAD), dev.put(padded(tc, np.uint16, SOLID))
    assert CL.yakamd_correct_decide_dev(k, c, d_tc, d_fix, nf, d_img, n, d_tal, ns) == 0, co._err()
    g_img, g_fix, g_tal = dev.get(d_img, room + PAD), dev.get(d_fix, nf * 32 + PAD), dev.get(d_tal, ns * 32 + PAD)
    assert (g_img[n:room] == 10).all() and (g_img[room:] == FILL).all() and (g_fix[nf * 32:] == FILL).all() and (g_tal[ns * 32:] == FILL).all()
    return g_fix[:nf * 32].view(K.FIX_DTYPE), g_tal[:ns * 32].view(K.TALLY_DTYPE), g_img[:n].tobytes()


def hand_reads():
    names = sorted(n for n in CASES if CASES[n][1] == 1)
    return names, [CASES[n][0] for n in names]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """{name: (the .yak file, k, x, c)} of the oracle's dumps: the hand table, one of k = 31 and the planted reads'"""
    d = tmp_path_factory.mktemp("correct_tables")
    out = {}
    fn = str(d / "hand.yak")
    out["hand"] = (fn, 5) + K.oracle_table([s.encode() for s in HAND_TABLE], 5, fn)
    k, seed = PLANTED[0]
    clean, bad = K.planted(k, seed)
    fn = str(d / "planted.yak")
    out["planted"] = (fn, k) + K.oracle_table([r.encode() for r in clean], k, fn, pre=12)
    clean31 = K.planted(31, 2, n_reads=20)[0]
    fn = str(d / "k31.yak")
    out["k31"] = (fn, 31) + K.oracle_table([r.encode() for r in clean31], 31, fn, pre=12)
    return out


def inputs(tables, which):
    """(the table, the reads, min_cnt) of a named input"""
    if which == "hand":
        return tables["hand"], hand_reads()[1], 2
    if which == "planted":
        return tables["planted"], K.planted(*PLANTED[0])[1], 3
    return tables["k31"], K.planted(31, 2, n_reads=20)[1], 3


@pytest.mark.parametrize("which", ["hand", "planted", "k31"])
def test_trials_and_decisions_against_the_restatement(co, dev, tables, which):
    (fn, k, x, cx), reads, c = inputs(tables, which)
    img, offs, lens = K.image([r.encode() for r in reads])
    d = K.flat(img, offs, lens, k, c, 1, x, cx)
    assert len(d["recs0"]) > 10
    assert trials_dev(co, dev, img, d["recs0"], k) == d["trials"]
    recs, tal, out = decide_dev(co, dev, img, d["recs0"], d["tal0"], d["tc"], k, c)
    bad = [i for i in range(len(recs)) if recs[i] != d["recs"][i]]
    assert not bad, (bad[:4], recs[bad[:4]], d["recs"][bad[:4]])
    assert (tal == d["tal"]).all() and out == d["img"]


def test_trials_and_decisions_refuse_a_damaged_record(co, dev, tables):
    (fn, k, x, cx), reads, c = inputs(tables, "hand")
    img, offs, lens = K.image([r.encode() for r in reads])
    d = K.flat(img, offs, lens, k, c, 1, x, cx)
    CL = co.lib()
    for field, value in (("at", len(img) + 5), ("en", int(d["recs0"][0]["st"]) + k + 1), ("p", int(d["recs0"][0]["p"]) + 1), ("at", int(offs[1]) - 1)):
        recs = d["recs0"].copy()
        recs[0][field] = value
        trials_dev(co, dev, img, recs, k, want_rc=-1)
        assert b"do not lie inside the image" in CL.yakamd_correct_last_error()
        d_img, d_fix, d_tal = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10)), dev.put(recs), dev.put(d["tal0"])
        assert CL.yakamd_correct_decide_dev(k, c, dev.put(padded(d["tc"], np.uint16, SOLID)), d_fix, len(recs), d_img, len(img), d_tal, len(lens)) == -1
        assert b"do not lie inside the image" in CL.yakamd_correct_last_error()
        dev.free()
    recs = d["recs0"].copy()
    recs[0]["seq"] = len(lens)                                   # a sequence that is none: the decisions refuse it
    d_img, d_fix, d_tal = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10)), dev.put(recs), dev.put(d["tal0"])
    assert CL.yakamd_correct_decide_dev(k, c, dev.put(padded(d["tc"], np.uint16, SOLID)), d_fix, len(recs), d_img, len(img), d_tal, len(lens)) == -1


# ---- one image in place ----
class Table:
    def __init__(self, ya, fn):
        self.L = ya.lib()
        self.h = self.L.yak_ch_restore(fn.encode())
        assert self.h, ya._err()

    def close(self):
        if self.h:
            self.L.yak_ch_destroy(self.h)
            self.h = None


def image_dev(co, dev, h, img, offs, lens, c, e, cap):
    CL = co.lib()
    n, ns = len(img), len(lens)
    room = K.up16(n)
    d_img = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10), PAD)
    d_off, d_len = dev.put(np.asarray(offs, np.uint64)), dev.put(np.asarray(lens, np.uint32))
    d_fix, d_tal = dev.put(np.full(cap * 32, FILL, np.uint8), PAD), dev.put(np.full(ns * 32, FILL, np.uint8), PAD)
    r = CL.yakamd_correct_image_dev(h, c, e, d_img, n, d_off, d_len, ns, d_fix, cap, d_tal)
    assert r >= 0, co._err()
    g_img, g_fix, g_tal = dev.get(d_img, room + PAD), dev.get(d_fix, cap * 32 + PAD), dev.get(d_tal, ns * 32 + PAD)
    assert (g_img[n:room] == 10).all() and (g_img[room:] == FILL).all() and (g_fix[cap * 32:] == FILL).all() and (g_tal[ns * 32:] == FILL).all()
    return r, g_fix[:cap * 32], g_tal[:ns * 32].view(K.TALLY_DTYPE), g_img[:n].tobytes()


@pytest.mark.parametrize("which", ["hand", "planted", "k31"])
def test_image_dev_against_the_three_calls_and_the_restatement(ya, co, dev, tables, which):
    (fn, k, x, cx), reads, c = inputs(tables, which)
    img, offs, lens = K.image([r.encode() for r in reads])
    L, CL = ya.lib(), co.lib()
    T = Table(ya, fn)
    try:
        for e in (1, 3):
            d = K.flat(img, offs, lens, k, c, e, x, cx)
            nf = len(d["recs"])
            # the three calls, with the library's own lookups between them
            d_img = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10))
            d_cnt = dev.put(np.zeros(K.up16(len(img)), np.uint16))
            assert L.yakamd_lookup_dev(T.h, d_img, len(img), d_cnt) == 0, ya._err()
            t = dev.get(d_cnt, 2 * len(img)).view(np.uint16)
            assert (t == d["t"]).all(), "the lookup is not the dump's"
            r, fix, tal = find_dev(co, dev, t, offs, lens, k, c, e)
            assert r == nf and (fix.view(K.FIX_DTYPE) == d["recs0"]).all() and (tal == d["tal0"]).all()
            tr = trials_dev(co, dev, img, d["recs0"], k)
            assert tr == d["trials"]
            d_tr, d_tc = dev.put(np.frombuffer(tr, np.uint8)), dev.put(np.zeros(max(len(tr), 16), np.uint16))
            assert L.yakamd_lookup_dev(T.h, d_tr, len(tr), d_tc) == 0, ya._err()
            tc = dev.get(d_tc, 2 * len(tr)).view(np.uint16)
            assert (tc == d["tc"]).all()
            recs, tal, out = decide_dev(co, dev, img, d["recs0"], d["tal0"], tc, k, c)
            assert (recs == d["recs"]).all() and (tal == d["tal"]).all() and out == d["img"]
            dev.free()
            # the one call: with room for the records, with too little, and once more on its own output
            r, fix, tal, out = image_dev(co, dev, T.h, img, offs, lens, c, e, nf)
            assert r == nf and (fix.view(K.FIX_DTYPE) == d["recs"]).all() and (tal == d["tal"]).all() and out == d["img"]
            r, fix, tal, out = image_dev(co, dev, T.h, img, offs, lens, c, e, max(nf - 1, 0))
            assert r == nf and (fix == FILL).all() and (tal == d["tal"]).all() and out == d["img"]
            left = d["recs"][d["recs"]["why"] != K.DONE]
            r, fix, tal2, out2 = image_dev(co, dev, T.h, d["img"], offs, lens, c, e, nf)
            assert r == len(left) and fix[:32 * r].tobytes() == left.tobytes() and out2 == d["img"] and not tal2["n_fixed"].any()
            assert (tal2["n_weak"] == d["tal"]["n_weak_after"]).all() and (tal2["n_weak_after"] == tal2["n_weak"]).all()
            dev.free()
    finally:
        T.close()


def test_empty_image_and_image_without_candidates_by_the_tally(ya, co, dev, tables):
    """no candidates: neither the trials nor the decisions are launched, and the table is looked up once; no bytes: nothing is launched"""
    fn, k, x, cx = tables["hand"]
    L, CL = ya.lib(), co.lib()
    T = Table(ya, fn)
    try:
        img, offs, lens = K.image([G.encode(), HAND_TABLE[2].encode(), b"ACG", b""])
        CL.yakamd_correct_tally_reset()
        with PU.tally(L, device=False) as base:
            r, fix, tal, out = image_dev(co, dev, T.h, img, offs, lens, 2, 1, 4)
        assert r == 0 and out == img and (fix == FILL).all() and [tuple(t)[:7] for t in tal] == [(26, 0, 0, 0, 0, 0, 0)] * 2 + [(0,) * 7] * 2
        assert co.tally() == {"k_cor_find<COUNT>": 1, "k_cor_tile_scan": 1, "k_cor_find<EMIT>": 0, "k_cor_trials": 0, "k_cor_decide": 0}
        assert base == {"k_lookup<unsignedshort,false>": 1}
        CL.yakamd_correct_tally_reset()
        with PU.tally(L, device=False) as base:
            r, fix, tal, out = image_dev(co, dev, T.h, b"", [0, 0], [0, 0], 2, 1, 4)
            assert CL.yakamd_correct_find_dev(5, 2, 1, None, 0, None, None, 0, None, 0, None) == 0
        assert r == 0 and (fix == FILL).all() and not any(co.tally().values()) and base == {} and [tuple(t)[:7] for t in tal] == [(0,) * 7] * 2
        # and with candidates every kernel of the tally runs, the table is looked up twice
        img, offs, lens = K.image([r.encode() for r in hand_reads()[1]])
        CL.yakamd_correct_tally_reset()
        with PU.tally(L, device=False) as base:
            r = image_dev(co, dev, T.h, img, offs, lens, 2, 1, 64)[0]
        assert r > 5 and co.tally() == {n: 1 for n in KERNELS} and base == {"k_lookup<unsignedshort,false>": 2}
    finally:
        T.close()


# ---- the command ----
def records_of(names, reads, fastq):
    return [(n, "c %d" % i if i % 2 else "", "I" * len(r) if fastq else "") for i, (n, r) in enumerate(zip(names, reads))]


@pytest.mark.parametrize("which", ["hand", "planted"])
def test_command_byte_for_byte_in_any_chunking(ya, co, tables, tmp_path, which):
    """yakamd_correct through yak_amd.correct and the CLI: both texts in three chunk sizes down to one read per chunk, from FASTA, FASTQ and gzip"""
    (fn, k, x, cx), reads, c = inputs(tables, which)
    names = hand_reads()[0] if which == "hand" else ["read%d" % i for i in range(len(reads))]
    img, offs, lens = K.image([r.encode() for r in reads])
    d = K.flat(img, offs, lens, k, c, 1, x, cx)
    out = [d["img"][int(o):int(o) + int(L)].decode() for o, L in zip(offs, lens)]
    if which == "planted":
        assert out == K.planted(*PLANTED[0])[0][::3]              # the planted reads restored
    for form in ("fa", "fq", "fa.gz"):
        recs = records_of(names, reads, form == "fq")
        text = K.reads_text(recs, reads)
        src = str(tmp_path / ("in." + form))
        with open(src, "wb") as f:
            f.write(gzip.compress(text) if form.endswith(".gz") else text)
        want_reads = K.reads_text(recs, out)
        for chunk, lf in ((None, True), (1000, True), (1, True), (None, False)):
            got_reads, got_rep = co.correct(fn, src, min_cnt=c, list_fixed=lf, chunk_size=chunk)
            assert got_reads == want_reads and got_rep == K.flat_report(names, d, lens, k, c, 1, lf), (form, chunk, lf)
        if form != "fq":
            continue
        rep = str(tmp_path / "rep.txt")
        r = subprocess.run([CLI, "correct", "-c", str(c), "-l", "-K", "700", "-r", rep, fn, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and r.stdout == want_reads and open(rep, "rb").read() == K.flat_report(names, d, lens, k, c, 1, True), r.stderr
        r = subprocess.run([CLI, "correct", "-c", str(c), "-s", fn, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and r.stdout == K.flat_report(names, d, lens, k, c, 1, False), r.stderr
    # min_run 3 through the command
    d3 = K.flat(img, offs, lens, k, c, 3, x, cx)
    assert co.correct(fn, src, min_cnt=c, min_run=3, list_fixed=True)[1] == K.flat_report(names, d3, lens, k, c, 3, True)
    # idempotence on the device, and n_weak_after against a lookup of the output
    once = str(tmp_path / "once.fa")
    co.correct(fn, src, out_fn=once, min_cnt=c)
    again, rep2 = co.correct(fn, once, min_cnt=c, list_fixed=True)
    assert again == open(once, "rb").read() and b"\nX\t" not in rep2
    L = ya.lib()
    T, dv = Table(ya, fn), Dev(L)
    try:
        d_cnt = dv.put(np.zeros(K.up16(len(img)), np.uint16))
        assert L.yakamd_lookup_dev(T.h, dv.put(padded(np.frombuffer(d["img"], np.uint8), np.uint8, 10)), len(img), d_cnt) == 0
        t = dv.get(d_cnt, 2 * len(img)).view(np.uint16).astype(np.int64)
        weak = (t != K.NO) & (t < c)
        s_lines = [ln.split("\t") for ln in co.correct(fn, src, min_cnt=c, stats_only=True)[1].decode().splitlines() if ln.startswith("S\t")]
        assert [int(f[9]) for f in s_lines] == [int(weak[int(o):int(o) + int(n)].sum()) for o, n in zip(offs, lens)]
    finally:
        dv.free()
        T.close()


def test_refusals_with_a_table(ya, co, dev, tables, tmp_path):
    fn, k, x, cx = tables["hand"]
    L, CL = ya.lib(), co.lib()
    err = CL.yakamd_correct_last_error
    reads = tmp_path / "r.fa"
    reads.write_text(">r\n%s\n" % mut(G, 12))
    out, rep = tmp_path / "o.fa", tmp_path / "rep.txt"
    T = ya.Table(5, 10, 4, 0)                                    # a resident table of the same k-mers: it can open a pass
    try:
        T.count_pass_host(1, K.image([s.encode() for s in HAND_TABLE])[0])
        call = lambda o, src=reads: CL.yakamd_correct(C.byref(o), T.h, str(src).encode(), str(out).encode(), str(rep).encode())
        for kw, msg in ((dict(min_cnt=0), b"min_cnt"), (dict(min_cnt=1024), b"min_cnt"), (dict(min_run=0), b"min_run"), (dict(min_run=6), b"min_run"), (dict(chunk_size=0), b"chunk_size")):
            assert call(co.options(**kw)) == -1 and msg in err() and not out.exists() and not rep.exists(), kw
        assert call(co.options(), tmp_path / "none.fa") == -1 and b"cannot read" in err() and not out.exists() and not rep.exists()
        img, offs, lens = K.image([mut(G, 12).encode()])
        d_img, d_off, d_len = dev.put(padded(np.frombuffer(img, np.uint8), np.uint8, 10)), dev.put(offs), dev.put(lens)
        one = lambda c, e, p=d_img: CL.yakamd_correct_image_dev(T.h, c, e, p, len(img), d_off, d_len, 1, None, 0, None)
        assert one(0, 1) == -1 and b"min_cnt" in err() and one(2, 6) == -1 and b"min_run" in err() and one(2, 1, d_img + 8) == -1 and b"16-byte aligned" in err()
        assert (dev.get(d_img, len(img)).tobytes()) == img, "a refused call wrote"
        assert L.yakamd_ch_set_hpc(T.h, 1) == 0
        assert one(2, 1) == -1 and b"homopolymer-compressed" in err() and call(co.options(min_cnt=2)) == -1 and b"homopolymer-compressed" in err() and not out.exists()
        assert L.yakamd_ch_set_hpc(T.h, 0) == 0
        assert L.yakamd_pass_begin(T.h, 0) == 0                  # an open pass: what the lookup refuses
        assert one(2, 1) == -1 and b"open pass" in err() and call(co.options(min_cnt=2)) == -1 and not out.exists()
        assert L.yakamd_pass_end(T.h) >= 0
        assert one(2, 1) == 1 and call(co.options(min_cnt=2)) == 0 and out.read_text() == ">r\n%s\n" % G
    finally:
        T.close()
    T = ya.Table(33, 10, 4, 0)
    try:
        T.count_pass_host(1, (G * 2).encode() + b"\n")
        assert CL.yakamd_correct_image_dev(T.h, 2, 1, None, 0, None, None, 0, None, 0, None) == -1 and b"k must be below 32" in err()
    finally:
        T.close()
