"""`yak chkerr` on the device (k_lookup's chkerr mode + the k_te_* run finder + yakamd_chkerr): byte-equal to the reference's
`chkerr -t1` on the stored fixtures for every option set at k = 21 and 41, the same bytes in any chunking, from stdin and from .gz; the
streak export equal to the Python restatement on random and adversarial arrays; a key equal to the empty-slot value at k = 41; refusals."""
import ctypes as C
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import chkerr_util as U
import gen_golden_chkerr as G
from test_gpu_triobin import Dev

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
NOKMER = 0xFF
TILE = 4096                               # positions per workgroup of k_te_runs


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "chkerr.json")))


@pytest.fixture(scope="module")
def ce(tmp_path_factory, gold):
    """the fixture inputs and, per k, the table counted on the device"""
    d = tmp_path_factory.mktemp("chkerr")
    p = G.make_inputs(str(d))
    tabs = {}

    def table(k):
        if k not in tabs:
            fn = str(d / ("reads_k%d.yak" % k))
            subprocess.run([CLI, "count", "-k%d" % k] + gold["count_args"] + ["-o", fn, p["reads.fa"]], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            tabs[k] = fn
        return tabs[k]
    return d, p, table


def cli(opts, tab, fa, **kw):
    return subprocess.run([CLI, "chkerr"] + opts + [tab, fa], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                          timeout=600, **kw).stdout


def lib_kw(opts):
    kw = {}
    for o in opts:
        if o.startswith("-c"): kw["min_cnt"] = int(o[2:])
        if o.startswith("-s"): kw["min_streak"] = int(o[2:])
    return kw


def test_table_equals_reference(gold, ce):
    _, _, table = ce
    for ks, case in gold["cases"].items():
        assert G.md5(table(int(ks[1:]))) == case["table_md5"], ks


@pytest.mark.parametrize("ks", ["k21", "k41"])
@pytest.mark.parametrize("name", list(G.OPTION_SETS))
def test_cli_and_library_equal_golden(gold, ce, ks, name):
    import yak_amd
    _, p, table = ce
    k, opts = int(ks[1:]), gold["option_sets"][name]
    want = gold["cases"][ks]["out"]["asm.fa:" + name]
    got = cli(opts, table(k), p["asm.fa"])
    assert G.expected(want, got), got.decode()[-2000:]
    assert yak_amd.chkerr(table(k), p["asm.fa"], **lib_kw(opts)) == got


@pytest.mark.parametrize("chunk", [1, 30000, 400000])
def test_chunks_do_not_show(gold, ce, chunk):
    import yak_amd
    _, p, table = ce
    for ks, name in (("k21", "sm1"), ("k41", "default")):
        got = yak_amd.chkerr(table(int(ks[1:])), p["asm.fa"], chunk=chunk, **lib_kw(gold["option_sets"][name]))
        assert G.expected(gold["cases"][ks]["out"]["asm.fa:" + name], got), (ks, name, chunk)
    got = cli(["-K", str(chunk), "-s-1"], table(21), p["asm.fa"])
    assert G.expected(gold["cases"]["k21"]["out"]["asm.fa:sm1"], got)


def test_stdin_and_gz(gold, ce):
    d, p, table = ce
    gz = str(d / "asm.fa.gz")
    data = open(p["asm.fa"], "rb").read()
    with gzip.open(gz, "wb") as f:
        f.write(data)
    want = gold["cases"]["k41"]["out"]["asm.fa:c1s0"]
    assert G.expected(want, cli(["-c1", "-s0"], table(41), gz))
    assert G.expected(want, cli(["-c1", "-s0"], table(41), "-", input=data))
    import yak_amd
    assert G.expected(want, yak_amd.chkerr(table(41), gz, min_cnt=1, min_streak=0))


@pytest.mark.skipif(not os.path.exists(YAK_ON_AMD), reason="reference caller not built")
def test_reference_caller_on_library(ce):
    """the reference's own chkerr.c on the library's host yak_ch_get"""
    _, p, table = ce
    for k in (21, 41):
        for opts in ([], ["-c0"], ["-s-1"]):
            assert G.ref_chkerr(YAK_ON_AMD, table(k), p["asm.fa"], opts) == cli(opts, table(k), p["asm.fa"]), (k, opts)


# ---- the streak export against the restatement ----
def check_streaks(seqs, min_streak, lead=0):
    """lay the low-byte arrays out with a NOKMER byte after each (after `lead` NOKMER bytes), list the streaks on the device, compare"""
    import yak_amd
    L = yak_amd.lib()
    off = np.zeros(len(seqs), np.uint64)
    buf, at = [np.full(lead, NOKMER, np.uint8)], lead
    for j, s in enumerate(seqs):
        off[j] = at
        buf.append(np.asarray(s, np.uint8)); buf.append(np.array([NOKMER], np.uint8))
        at += len(s) + 1
    low = np.concatenate(buf)
    dev = Dev(L)
    d_sk, n_sk, n_only = C.c_void_p(), C.c_int64(-1), C.c_int64(-1)
    try:
        d_low, d_off = dev.put(low), dev.put(off)
        assert L.yakamd_chkerr_streaks_dev(min_streak, d_low, d_off, len(seqs), len(low), C.byref(d_sk), C.byref(n_sk), None) == 0, yak_amd._err()
        sk = dev.get(d_sk.value, n_sk.value * 4, np.uint32).reshape(-1, 4) if n_sk.value else np.zeros((0, 4), np.uint32)
        assert L.yakamd_chkerr_streaks_dev(min_streak, d_low, d_off, len(seqs), len(low), None, C.byref(n_only), None) == 0
        assert n_only.value == n_sk.value
    finally:
        L.yakamd_dev_free(d_sk.value)
        dev.free()
    want = U.low_runs(low, off.tolist(), [len(s) for s in seqs], min_streak)
    assert [tuple(x) for x in sk.tolist()] == want
    return len(want)


def runs(rng, n, mean):
    if n == 0:
        return np.zeros(0, np.uint8)
    ln = rng.geometric(1.0 / mean, size=max(8, int(n / mean * 2) + 8))
    while ln.sum() < n:
        ln = np.concatenate((ln, ln))
    return np.repeat(rng.choice(np.array([1, 0, NOKMER], np.uint8), size=len(ln)), ln)[:n]


@pytest.mark.parametrize("min_streak", [-1, 0, 5, 100])
def test_streaks_random(min_streak):
    rng = np.random.default_rng(min_streak + 10)
    seqs = [runs(rng, int(n), float(m)) for n, m in zip(rng.integers(0, 6000, 1500), rng.choice([1.5, 4, 30, 300], 1500))]
    assert check_streaks(seqs, min_streak, lead=int(rng.integers(0, 40))) > 100


def test_streaks_tile_boundaries_and_whole_array():
    f = np.zeros(12 * TILE, np.uint8)
    for st, en in [(0, 1), (15, 16), (16, 32), (TILE - 1, TILE + 1), (2 * TILE, 5 * TILE), (8 * TILE - 1, 8 * TILE), (11 * TILE - 1, 12 * TILE)]:
        f[st:en] = 1
    for lead in (0, 1, 15, TILE - 1):
        for ms in (-1, 0, 1, TILE):
            check_streaks([f, f[: 5 * TILE], f[TILE:]], ms, lead=lead)
    whole = np.ones(3 * TILE * 100 + 7, np.uint8)
    assert check_streaks([whole], 5) == 1
    assert check_streaks([whole], len(whole) - 1) == 1 and check_streaks([whole], len(whole)) == 0
    assert check_streaks([whole], 2**31 - 1) == 0                   # saturated: no overflow of min_streak + 1


def test_streaks_thousands_of_empty_records_and_a_long_one():
    rng = np.random.default_rng(3)
    seqs = [np.zeros(0, np.uint8)] * 5000 + [runs(rng, 2_000_000, 50.0)] + [runs(rng, int(n), 2.0) for n in rng.integers(0, 4, 20000)]
    assert check_streaks(seqs, -1) > 10000
    assert check_streaks(seqs, 3) > 1000


# ---- a stored key equal to the empty-slot value at k >= 32 ----
def test_empty_slot_key_at_k41(tmp_path):
    """a YAK_LOAD_ALL table at k = 41 whose home slot of a real k-mer holds a key equal to YK_EMPTY (all ones: hash bits all ones at count
    1023): the real key is placed behind it, and the probe must step over the full slot"""
    k, pre, bits, cap = 41, 10, 3, 8
    empty_home = U.h2b(0xFFFFFFFF, bits)
    rng = np.random.default_rng(41)
    while True:                                                     # a k-mer whose sub-table is 1023 and whose home slot is empty_home's
        s = bytes(rng.choice(list(b"ACGT"), k).tolist())
        h = U.kmer_hash(s, k)
        kid = (h >> pre) & ((1 << 54) - 1)
        if h & 1023 == 1023 and U.h2b(kid & 0xFFFFFFFF, bits) == empty_home and kid != (1 << 54) - 1:
            break
    body = bytearray(b"YAK\x02" + struct.pack("<3I", k, pre, 10))
    for p in range(1 << pre):
        if p == 1023:                                               # file order = insertion order: the all-ones key first
            body += struct.pack("<2I", cap, 2) + struct.pack("<2Q", (1 << 64) - 1, kid << 10 | 7)
        else:
            body += struct.pack("<2I", cap, 0)
    tab = str(tmp_path / "empty_slot_k41.yak")
    open(tab, "wb").write(bytes(body))
    fa = str(tmp_path / "one.fa")
    open(fa, "wb").write(b">hit\n" + s + b"\n>miss\n" + U_other(s) + b"\n")
    want = b"miss\t0\t41\t1\n"                                       # count 7 is not below 3; the other k-mer is absent
    assert cli(["-s0"], tab, fa) == want
    assert cli(["-s0", "-c8"], tab, fa) == b"hit\t0\t41\t1\n" + want
    if os.path.exists(G.REF_YAK):
        assert G.ref_chkerr(G.REF_YAK, tab, fa, ["-s0"]) == want


def U_other(s):
    """the k-mer with its middle base changed"""
    b = bytearray(s)
    m = len(b) // 2
    b[m] = b"ACGT"[(b"ACGT".index(b[m]) + 1) & 3]
    return bytes(b)


# ---- refusals ----
def test_sharded_table_refused(ce, monkeypatch, tmp_path):
    import yak_amd
    L = yak_amd.lib()
    _, p, _ = ce
    monkeypatch.setenv("YAKAMD_GPUS", "2"); monkeypatch.setenv("YAKAMD_GPU_LIST", "0,0")
    co = yak_amd.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k = 21
    h = L.yak_count(p["reads.fa"].encode(), C.byref(co), None)
    assert h, yak_amd._err()
    try:
        assert L.yakamd_last_sweeps() == 2
        o = yak_amd.CeoptT()
        L.yakamd_ceopt_init(C.byref(o))
        assert L.yakamd_chkerr(C.byref(o), h, p["asm.fa"].encode(), str(tmp_path / "o.txt").encode()) == -1
        dev = Dev(L)
        try:
            img = dev.put(np.frombuffer(b"ACGT" * 16, np.uint8))
            assert L.yakamd_chkerr_lookup_dev(h, img, 64, 3, dev.empty(64)) == -1
            assert b"sharded" in L.yakamd_last_error()
        finally:
            dev.free()
    finally:
        L.yak_ch_destroy(h)
