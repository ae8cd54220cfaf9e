"""`yak trioeval` on the device (k_lookup + the k_te_* streak kernels + yakamd_trioeval): byte-equal to the reference's
`trioeval -t1` on the stored fixtures, chunked like bseq_read, and the streak reduction equal to a Python restatement of
trioeval.c:89-116 on random and adversarial flag arrays."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import gen_golden_trioeval as G
from test_gpu_triobin import Dev

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
NOKMER = 0xFF
TILE = 4096                               # positions per workgroup of k_te_runs


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "trioeval.json")))


@pytest.fixture(scope="module")
def trio(tmp_path_factory, gold):
    """the fixture inputs and, per k, the parents' tables counted on the device"""
    d = tmp_path_factory.mktemp("trioeval")
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


def cli(opts, pat, mat, fa):
    return subprocess.run([CLI, "trioeval"] + opts + [pat, mat, fa], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def lib_kw(opts):
    kw = {}
    for o in opts:
        if o.startswith("-c"): kw["min_cnt"] = int(o[2:])
        if o.startswith("-d"): kw["mid_cnt"] = int(o[2:])
        if o.startswith("-n"): kw["min_n"] = int(o[2:])
        if o == "-e": kw["print_err"] = True
        if o == "-F": kw["print_frag"] = False
    return kw


def test_parent_tables_equal_reference(gold, trio):
    _, table = trio
    for ks, case in gold["cases"].items():
        for who in ("pat", "mat"):
            assert G.md5(table(int(ks[1:]), who)) == case[who + "_md5"], (ks, who)


@pytest.mark.parametrize("ks", ["k21", "k41"])
@pytest.mark.parametrize("fa", G.ASSEMBLIES)
@pytest.mark.parametrize("name", list(G.OPTION_SETS))
def test_cli_and_library_equal_golden(gold, trio, ks, fa, name):
    import yak_amd
    p, table = trio
    k, opts = int(ks[1:]), gold["option_sets"][name]
    want = gold["cases"][ks]["out"]["%s:%s" % (fa, name)]
    pat, mat = table(k, "pat"), table(k, "mat")
    got = cli(opts, pat, mat, p[fa])
    assert G.expected(want, got), got.decode()[-2000:]
    assert yak_amd.trioeval(pat, mat, p[fa], **lib_kw(opts)) == got


@pytest.mark.parametrize("chunk", [1, 30000, 400000])
def test_chunks_close_like_bseq_read(gold, trio, chunk):
    """per chunk the F / E lines of its sequences, then its S lines: the one-chunk output regrouped where bseq_read closes chunks"""
    import yak_amd
    p, table = trio
    pat, mat = table(21, "pat"), table(21, "mat")
    whole = yak_amd.trioeval(pat, mat, p["asm.fa"], print_err=True)
    assert G.expected(gold["cases"]["k21"]["out"]["asm.fa:e"], whole)
    lines = whole.split(b"\n")[:-1]
    head, body, foot = lines[:6], lines[6:-3], lines[-3:]
    fe = [l for l in body if l[:2] in (b"F\t", b"E\t")]
    s_lines = [l for l in body if l.startswith(b"S\t")]
    want, acc, group = list(head), 0, []
    for i, l in enumerate(s_lines):                  # bseq.c:54: a chunk closes once its bases reach the chunk size
        group.append(l)
        acc += int(l.split(b"\t")[-1])
        if acc >= chunk or i == len(s_lines) - 1:
            names = {g.split(b"\t")[1] for g in group}
            want += [x for x in fe if x.split(b"\t")[1] in names] + group
            group, acc = [], 0
    want += foot
    assert yak_amd.trioeval(pat, mat, p["asm.fa"], print_err=True, chunk=chunk) == b"".join(x + b"\n" for x in want)


@pytest.mark.skipif(not os.path.exists(YAK_ON_AMD), reason="reference caller not built")
def test_reference_caller_on_library(trio):
    """the reference's own trioeval.c on the library's host yak_ch_get"""
    p, table = trio
    for k in (21, 41):
        pat, mat = table(k, "pat"), table(k, "mat")
        for opts in (["-e"], ["-n1"], ["-c1", "-d2"]):
            assert G.ref_trioeval(YAK_ON_AMD, pat, mat, p["asm.fa"], opts) == cli(opts, pat, mat, p["asm.fa"]), (k, opts)


def test_table_with_counts_above_15_fails(trio):
    """a table restored in YAK_LOAD_ALL mode keeps its counts: trioeval must refuse it with a message"""
    import yak_amd
    L = yak_amd.lib()
    p, table = trio
    h = L.yak_ch_restore(table(21, "pat").encode())
    assert h
    try:
        o = yak_amd.TeoptT()
        L.yakamd_teopt_init(C.byref(o))
        assert L.yakamd_trioeval(C.byref(o), h, p["asm.fa"].encode(), os.devnull.encode()) == -1
        assert b"above 15" in L.yakamd_last_error()
    finally:
        L.yak_ch_destroy(h)


# ---- the streak reduction against trioeval.c:89-116 ----
def te_ref(f, k, min_n, j, streaks):
    """trioeval.c:89-116 on one sequence's flags: [d0, d1, c0, c1, c2, c3]; appends (j, l, i, type) per streak"""
    t = np.where(f == 2, 1, np.where(f == 8, 2, 0))
    d, c = [0, 0], [0, 0, 0, 0]
    if len(t) == 0:
        return d + c
    cut = np.flatnonzero(t[1:] != t[:-1]) + 1
    last = 0
    for l, i in zip(np.concatenate(([0], cut)).tolist(), np.concatenate((cut, [len(t)])).tolist()):
        ty = int(t[l])
        if ty > 0 and i - l >= min_n:
            n, cc = (i - l + k - 1) // k, ty - 1
            c[cc << 1 | cc] += n - 1
            d[cc] += n
            if last > 0:
                c[(last - 1) << 1 | cc] += 1
            streaks.append((j, l, i, ty))
            last = ty
    return d + c


def runs(rng, n, mean, alphabet=(2, 8, 0, 10, NOKMER)):
    """n flags in runs of geometric length (mean `mean`) of values drawn from `alphabet`"""
    if n == 0:
        return np.zeros(0, np.uint8)
    m = max(1, int(n / mean * 1.5) + 8)
    ln = rng.geometric(1.0 / mean, size=m)
    while ln.sum() < n:
        ln = np.concatenate((ln, rng.geometric(1.0 / mean, size=m)))
    v = rng.choice(np.array(alphabet, np.uint8), size=len(ln))
    return np.repeat(v, ln)[:n]


def check_reduce(seqs, k, min_n, lead=0):
    """lay the sequences out with a NOKMER byte after each (after `lead` NOKMER bytes), reduce on the device, compare"""
    import yak_amd
    L = yak_amd.lib()
    off = np.zeros(len(seqs), np.uint64)
    buf, at = [np.full(lead, NOKMER, np.uint8)], lead
    for j, s in enumerate(seqs):
        off[j] = at
        buf.append(s); buf.append(np.array([NOKMER], np.uint8))
        at += len(s) + 1
    flags = np.concatenate(buf)
    lens = np.array([len(s) for s in seqs], np.uint32)
    dev = Dev(L)
    d_sk, n_sk = C.c_void_p(), C.c_int64(-1)
    try:
        d_f, d_off, d_len = dev.put(flags), dev.put(off), dev.put(lens)
        d_cnt = dev.empty(len(seqs) * 24)
        assert L.yakamd_trioeval_reduce_dev(k, min_n, d_f, d_off, d_len, len(seqs), len(flags), d_cnt, C.byref(d_sk), C.byref(n_sk), None) == 0, \
            yak_amd._err()
        got = dev.get(d_cnt, len(seqs) * 6, np.int32).reshape(-1, 6)
        sk = dev.get(d_sk.value, n_sk.value * 4, np.uint32).reshape(-1, 4) if n_sk.value else np.zeros((0, 4), np.uint32)
        n_plain = C.c_int64(-1)                       # without the list: the same counts
        assert L.yakamd_trioeval_reduce_dev(k, min_n, d_f, d_off, d_len, len(seqs), len(flags), d_cnt, None, C.byref(n_plain), None) == 0
        assert n_plain.value == n_sk.value
        assert (dev.get(d_cnt, len(seqs) * 6, np.int32).reshape(-1, 6) == got).all()
    finally:
        L.yakamd_dev_free(d_sk.value)
        dev.free()
    want_sk = []
    for j, s in enumerate(seqs):
        assert list(got[j]) == te_ref(s, k, min_n, j, want_sk), (j, len(s))
    assert [tuple(x) for x in sk.tolist()] == want_sk
    return len(want_sk)


@pytest.mark.parametrize("k,min_n", [(3, 2), (21, 2), (21, -1), (21, 1), (41, 5), (63, 2)])
def test_reduce_random(k, min_n):
    rng = np.random.default_rng(k * 100 + min_n)
    seqs = [runs(rng, int(n), float(m)) for n, m in zip(rng.integers(0, 6000, 1500), rng.choice([1.5, 4, 30, 300], 1500))]
    assert check_reduce(seqs, k, min_n, lead=int(rng.integers(0, 40))) > 1000


def test_reduce_tile_and_thread_boundaries():
    """runs that start or end exactly on a 16-position thread slice or a 4096-position tile, and runs spanning tiles"""
    f = np.zeros(12 * TILE, np.uint8)
    for st, en, v in [(0, 1, 2), (15, 16, 8), (16, 32, 2), (TILE - 1, TILE, 8), (TILE, 2 * TILE, 2), (2 * TILE, 2 * TILE + 1, 8),
                      (3 * TILE - 16, 3 * TILE + 16, 2), (3 * TILE + 16, 7 * TILE, 8), (7 * TILE, 7 * TILE + 2, 2),
                      (8 * TILE - 2, 8 * TILE - 1, 8), (8 * TILE - 1, 8 * TILE, 2), (9 * TILE + 1, 11 * TILE - 1, 2),
                      (11 * TILE - 1, 12 * TILE, 8)]:
        f[st:en] = v
    for lead in (0, 1, 15, TILE - 1):
        for min_n in (1, 2, 3):
            check_reduce([f, f[: 5 * TILE], f[TILE:]], 21, min_n, lead=lead)


def test_reduce_one_run_of_several_mb():
    f = np.full(6_000_000, 2, np.uint8)
    f[:7] = 0
    f[-3:] = 8
    assert check_reduce([f, np.full(TILE * 300 + 5, 8, np.uint8)], 21, 2) == 3


def test_reduce_alternating_types_every_position():
    f = np.tile(np.array([2, 8], np.uint8), 150_001)
    assert check_reduce([f, f[1:], f[:-1]], 21, 1) == 3 * len(f) - 2
    assert check_reduce([f], 21, 2) == 0


def test_reduce_many_tiny_sequences():
    rng = np.random.default_rng(5)
    k = 21
    seqs = [runs(rng, int(n), 3.0, (2, 8, NOKMER)) for n in rng.integers(0, k + 2, 100_000)]
    assert check_reduce(seqs, k, 1) > 10000


def test_reduce_50mb_single_sequence():
    rng = np.random.default_rng(50)
    f = runs(rng, 50_000_000, 400.0)
    assert check_reduce([f], 31, 2) > 10000
