"""`yak triobin` on the device (k_lookup + k_tb_reduce + yakamd_triobin): byte-equal to the reference's
`triobin -t1` on the stored fixtures and at -p13, per-position flags equal to the oracle's restatement (yko_lookup_image), and the
per-read reduction equal to a numpy restatement of triobin.c:74-100."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import gen_golden_triobin as G

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
NOKMER = 0xFF


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "triobin.json")))


@pytest.fixture(scope="module")
def trio(tmp_path_factory, gold):
    """the fixture inputs and, per k, the parents' tables counted on the device"""
    d = tmp_path_factory.mktemp("trio")
    p = G.make_inputs(str(d))
    tabs = {}

    def table(k, who):
        key = (k, who)
        if key not in tabs:
            fn = str(d / ("%s_k%d.yak" % (who, k)))
            subprocess.run([CLI, "count", "-k%d" % k] + gold["count_args"] + ["-o", fn, p[who + ".fa"]], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            tabs[key] = fn
        return tabs[key]
    return p, table


def test_parent_tables_equal_reference(gold, trio):
    _, table = trio
    for ks, case in gold["cases"].items():
        for who in ("pat", "mat"):
            assert G.md5(table(int(ks[1:]), who)) == case[who + "_md5"], (ks, who)


@pytest.mark.parametrize("ks,name", [("k21", n) for n in ("c1d2", "default", "p", "r05")] + [("k41", n) for n in ("c1d2", "default", "p", "r05")])
def test_cli_and_library_equal_golden(gold, trio, ks, name):
    p, table = trio
    k, opts = int(ks[1:]), gold["option_sets"][name]
    want = gold["cases"][ks]["out"][name]
    pat, mat = table(k, "pat"), table(k, "mat")
    got = subprocess.run([CLI, "triobin"] + opts + [pat, mat, p["child.fa"]], check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, timeout=600).stdout
    assert G.expected(want, got)
    import yak_amd
    kw = dict(print_diff="-p" in opts)
    for o in opts:
        if o.startswith("-c"): kw["min_cnt"] = int(o[2:])
        if o.startswith("-d"): kw["mid_cnt"] = int(o[2:])
        if o.startswith("-r"): kw["ratio"] = float(o[2:])
    assert yak_amd.triobin(pat, mat, p["child.fa"], **kw) == got


def test_chunks_close_like_bseq_read(gold, trio):
    """with small chunks the per-read lines do not change, and -p's D lines come chunk by chunk before that chunk's reads"""
    import yak_amd
    p, table = trio
    pat, mat = table(21, "pat"), table(21, "mat")
    case = gold["cases"]["k21"]["out"]
    assert G.expected(case["default"], yak_amd.triobin(pat, mat, p["child.fa"], chunk=20000))
    whole = yak_amd.triobin(pat, mat, p["child.fa"], print_diff=True)        # one chunk: the reference's bytes
    assert G.expected(case["p"], whole)
    lines = whole.split(b"\n")[:-1]
    dl = [l for l in lines if l.startswith(b"D\t")]
    summ = [l for l in lines if not l.startswith(b"D\t")]
    lens = [len(s) for _, s in _records(p["child.fa"])]
    want, at, acc, group = [], 0, 0, []
    for i, (l, n) in enumerate(zip(summ, lens)):        # bseq.c:54: a chunk closes once its bases reach the chunk size
        group.append(l)
        acc += n
        if acc >= 20000 or i == len(summ) - 1:
            names = {g.split(b"\t")[0] for g in group}
            want += [x for x in dl if x.split(b"\t")[1] in names] + group
            group, acc = [], 0
    got = yak_amd.triobin(pat, mat, p["child.fa"], print_diff=True, chunk=20000)
    assert got == b"".join(x + b"\n" for x in want)


@pytest.mark.skipif(not (os.path.exists(G.REF_YAK) and os.path.exists(YAK_ON_AMD)), reason="reference binaries not built")
def test_live_reference_and_reference_caller_on_library(gold, trio):
    p, table = trio
    for k in (21, 41):
        pat, mat = table(k, "pat"), table(k, "mat")
        for opts in (["-p"], ["-c1", "-d2"]):
            mine = subprocess.run([CLI, "triobin"] + opts + [pat, mat, p["child.fa"]], check=True, stdout=subprocess.PIPE,
                                  stderr=subprocess.DEVNULL, timeout=600).stdout
            assert G.ref_triobin(G.REF_YAK, pat, mat, p["child.fa"], opts) == mine
            assert G.ref_triobin(YAK_ON_AMD, pat, mat, p["child.fa"], opts) == mine


def _records(fn):
    out, name, seq = [], None, []
    for ln in open(fn, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            if name is not None:
                out.append((name, b"".join(seq)))
            name, seq = ln[1:].split()[0] if ln[1:].split() else b"", []
        elif ln:
            seq.append(ln)
    if name is not None:
        out.append((name, b"".join(seq)))
    return out


class Dev:
    def __init__(self, L):
        self.L, self.bufs = L, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.L.yakamd_dev_alloc(max(arr.nbytes, 16))
        assert p
        self.bufs.append(p)
        if arr.nbytes:
            assert self.L.yakamd_memcpy_h2d(p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def empty(self, nbytes):
        return self.put(np.zeros(nbytes, np.uint8))

    def get(self, p, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            assert self.L.yakamd_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)


@pytest.mark.parametrize("k", [21, 31, 32, 41])
def test_lookup_equals_host_mirror(trio, oracle, k):
    """per-position flags against the oracle's restatement (yko_lookup_image) on the oracle's own two TRIOBIN loads of the same files, and
    the library's table bytes against the oracle's"""
    import yak_amd
    L, O = yak_amd.lib(), oracle.lib()
    p, table = trio
    h = yak_amd.triobin_table(table(k, "pat"), table(k, "mat"), 1, 2)
    o = O.yko_ch_restore_core(None, table(k, "pat").encode(), 2, 1, 2)
    o = O.yko_ch_restore_core(o, table(k, "mat").encode(), 3, 1, 2)
    dev = Dev(L)
    try:
        out = C.POINTER(C.c_uint8)()
        n = L.yakamd_dump_mem(h, C.byref(out))
        assert n > 0 and C.string_at(out, n) == oracle.dump_bytes(o)
        C.CDLL(None).free(out)
        recs = _records(p["child.fa"])
        img = b"".join(s[:6000] + b"\n" for _, s in recs)           # every record, the long ones cut to 6 kb
        img += b"\n" * (-len(img) % 16)
        d_img = dev.put(np.frombuffer(img, np.uint8))
        d_flag = dev.empty(len(img))
        assert L.yakamd_triobin_lookup_dev(h, d_img, len(img), d_flag) == 0, yak_amd._err()
        got = dev.get(d_flag, len(img), np.uint8)
        want = oracle.lookup_image(o, img, 1)
        assert (got <= 15).sum() > 1000 and (got[got <= 15] > 0).sum() > 1000
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    finally:
        dev.free()
        L.yak_ch_destroy(h)
        O.yko_ch_destroy(o)


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference binary not built")
@pytest.mark.parametrize("k", [21, 41])
def test_live_reference_on_parents_counted_at_p13(gold, trio, oracle, k, tmp_path):
    """-p13: the parents' tables have 8192 sub-tables and the lookup reads its directory from global memory (pre >= 13).  (13 is the largest
    prefix length the library's flag-mode loads take)"""
    p, _ = trio
    tabs = []
    for who in ("pat", "mat"):
        fn, want = str(tmp_path / (who + ".yak")), str(tmp_path / (who + "_oracle.yak"))
        for exe, out in ((CLI, fn), (os.path.join(ROOT, "oracle", "yko"), want)):
            subprocess.run([exe, "count", "-k%d" % k, "-p13"] + gold["count_args"] + ["-o", out, p[who + ".fa"]], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        data = open(fn, "rb").read()
        assert data == open(want, "rb").read() and data[8:12] == (13).to_bytes(4, "little")
        tabs.append(fn)
    for opts in (["-p"], ["-c1", "-d2"], []):
        mine = subprocess.run([CLI, "triobin"] + opts + tabs + [p["child.fa"]], check=True, stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, timeout=600).stdout
        assert G.ref_triobin(G.REF_YAK, tabs[0], tabs[1], p["child.fa"], opts) == mine and len(mine) > 500


def reduce_ref(f, k):
    """triobin.c:74-100 restated: c[16], sc[2], nk of one read's flag array"""
    has = f != NOKMER
    c = np.bincount(f[has], minlength=16)[:16]
    ty = np.where(f == 2, 1, np.where(f == 8, 2, 0))
    sc = [0, 0]
    if len(f):
        b = np.flatnonzero(np.diff(ty)) + 1                     # the maximal runs of one type
        st = np.concatenate([[0], b])
        ln = np.concatenate([b, [len(f)]]) - st
        t = ty[st]
        for j in (1, 2):
            sc[j - 1] = int(ln[(t == j) & (ln >= k - 4)].sum())
    return list(c) + sc + [int(has.sum())]


def crafted_reads(k, rng):
    reads = []
    for t, v in ((1, 2), (2, 8)):
        for n in (n for n in (k - 4, k - 5, k - 3) if n > 0):
            r = np.full(200, 10, np.uint8)
            r[70:70 + n] = v                                  # a run of exactly n inside a read
            reads.append(r)
            reads.append(np.full(n, v, np.uint8))             # the whole read is the run
    r = np.full(300, 0, np.uint8)
    r[40:170] = 2; r[170:190] = 8; r[190:260] = 2               # runs across the 64-position steps, adjacent runs of both types
    reads.append(r)
    r = np.full(130, 2, np.uint8); r[64] = NOKMER               # a run broken exactly at a step boundary
    reads.append(r)
    reads += [np.zeros(0, np.uint8), np.array([2], np.uint8), np.array([NOKMER], np.uint8)]
    big = rng.choice(np.array([0, 2, 8, 10, 1, 4, NOKMER], np.uint8), size=1000000, p=[.2, .3, .3, .1, .04, .04, .02])
    big = np.repeat(big[:40000], 25)                            # runs of 25 and their multiples
    reads.append(big)
    vals = np.array(list(range(16)) + [NOKMER], np.uint8)
    for _ in range(3000):
        n = int(rng.choice([0, 1, 2, 5, 63, 64, 65, 127, 128, 129, 500, 3000]) if rng.random() < .5 else rng.integers(0, 20000))
        if rng.random() < .5:
            r = np.repeat(rng.choice(vals, size=n // 7 + 1), rng.integers(1, 60, size=n // 7 + 1))[:n]
        else:
            r = rng.choice(np.array([2, 8, 10, NOKMER], np.uint8), size=n)
        reads.append(r.astype(np.uint8))
    return reads


@pytest.mark.parametrize("k", [3, 21, 41])
def test_reduce_equals_restatement(k):
    import yak_amd
    L = yak_amd.lib()
    rng = np.random.default_rng(k)
    reads = crafted_reads(k, rng)
    order = rng.permutation(len(reads))                          # reads laid out in another order than their index: offsets are honoured
    off = np.zeros(len(reads), np.uint64)
    buf, at = [], 0
    for j in order:
        off[j] = at
        buf.append(reads[j]); buf.append(np.array([NOKMER], np.uint8))
        at += len(reads[j]) + 1
    flags = np.concatenate(buf)
    lens = np.array([len(r) for r in reads], np.uint32)
    assert lens.max() == 1000000
    dev = Dev(L)
    try:
        d_f, d_off, d_len = dev.put(flags), dev.put(off), dev.put(lens)
        d_cnt = dev.empty(len(reads) * 19 * 4)
        assert L.yakamd_triobin_reduce_dev(k, d_f, d_off, d_len, len(reads), d_cnt, None) == 0, yak_amd._err()
        got = dev.get(d_cnt, len(reads) * 19, np.int32).reshape(-1, 19)
    finally:
        dev.free()
    for j, r in enumerate(reads):
        assert list(got[j]) == reduce_ref(r, k), (j, len(r))


def test_table_with_counts_above_15_fails(trio):
    """a table restored in YAK_LOAD_ALL mode keeps its counts (here up to ~40): the lookup must refuse it with a message"""
    import yak_amd
    L = yak_amd.lib()
    p, table = trio
    h = L.yak_ch_restore(table(21, "pat").encode())
    assert h
    dev = Dev(L)
    try:
        img = b"".join(s + b"\n" for _, s in _records(p["child.fa"])[:4])
        img += b"\n" * (-len(img) % 16)
        d_img, d_flag = dev.put(np.frombuffer(img, np.uint8)), dev.empty(len(img))
        assert L.yakamd_triobin_lookup_dev(h, d_img, len(img), d_flag) != 0
        assert b"above 15" in L.yakamd_last_error()
        o = yak_amd.TboptT()
        L.yakamd_tbopt_init(C.byref(o))
        assert L.yakamd_triobin(C.byref(o), h, p["child.fa"].encode(), os.devnull.encode()) == -1
    finally:
        dev.free()
        L.yak_ch_destroy(h)
