"""The table commands on the device: `yak-amd print [-c]` (k_print on the table's device-side .yak body) byte-equal to the reference's stored
output on every fixture table, in any batching, to a pipe and to a file; yakamd_kmers_dev equal to the oracle's and the library's getseq
over whole tables and ranges; tables from yak_count(), yak_ch_merge() and a sharded count listed as the oracle says; k >= 32 refused;
`cntasm / recount / subtract / isec` md5-equal to the reference's stored tables."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import gen_golden_tablecmds as G
import tablecmds_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
SYN = os.path.join(ROOT, "tools", "yaksynth")
T = 600


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "tablecmds.json")))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, gold, oracle):
    d = str(tmp_path_factory.mktemp("tablecmds"))
    p = G.make_inputs(d)
    G.make_tables(CLI, d, p)
    assert {n: G.md5(f) for n, f in sorted(p.items())} == gold["inputs"]
    assert {n: G.md5(G.table_path(n, d)) for n in G.MADE_TABLES} == gold["tables"]
    return d, p


def cli_print(fn, counts, opts=(), check=True):
    r = subprocess.run([CLI, "print"] + (["-c"] if counts else []) + list(opts) + [fn], check=check, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=T)
    return r.stdout if check else r


# ---- print: the stored cases ----
@pytest.mark.parametrize("name", G.PRINT_TABLES)
def test_print_equals_golden(name, gold, inputs):
    import yak_amd
    fn = G.table_path(name, inputs[0])
    for counts, key in ((False, "plain"), (True, "counts")):
        got = cli_print(fn, counts)
        assert G.expected(gold["print"][name][key], got), (name, key, got[:300])
        assert yak_amd.print_kmers(fn, counts=counts) == got


@pytest.mark.skipif(not os.path.exists(YAK_ON_AMD), reason="reference caller not built")
def test_print_equals_reference_caller_on_library(inputs):
    for name in G.PRINT_TABLES:
        fn = G.table_path(name, inputs[0])
        assert G.ref_print(YAK_ON_AMD, fn, True) == cli_print(fn, True), name
        assert G.ref_print(YAK_ON_AMD, fn, False) == cli_print(fn, False), name


@pytest.mark.parametrize("name", ["nb_k15_fa", "nb_k27_p12", "digits", "sparse", "polyA"])
def test_batching_does_not_show(name, gold, inputs):
    import yak_amd
    fn = G.table_path(name, inputs[0])
    for counts, key in ((False, "plain"), (True, "counts")):
        for bb in (1, 5000, 70000, None):                         # 1: the floor, one sub-table per range
            assert G.expected(gold["print"][name][key], yak_amd.print_kmers(fn, counts=counts, batch_bytes=bb)), (name, key, bb)
        assert G.expected(gold["print"][name][key], cli_print(fn, counts, ["-B", "3000"]))


def test_pipe_equals_file(gold, inputs, tmp_path):
    fn = G.table_path("nb_k31", inputs[0])
    out = str(tmp_path / "o.txt")
    with open(out, "wb") as f:
        subprocess.run([CLI, "print", "-c", fn], check=True, stdout=f, stderr=subprocess.DEVNULL, timeout=T)
    r = subprocess.run("%s print -c %s 2>/dev/null | cat" % (CLI, fn), shell=True, check=True, stdout=subprocess.PIPE, timeout=T)
    assert open(out, "rb").read() == r.stdout and G.expected(gold["print"]["nb_k31"]["counts"], r.stdout)


def test_print_without_tighten_is_not_the_reference_listing(gold, inputs):
    """the table made for it lists differently when yak_ch_tighten is left out: the step is the command's, and it is seen"""
    import yak_amd
    fn = G.table_path("sparse", inputs[0])
    e = gold["print"]["sparse"]["counts"]
    loose = yak_amd.print_kmers(fn, counts=True, tighten=False)
    assert not G.expected(e, loose) and sorted(loose.splitlines()) == sorted(yak_amd.print_kmers(fn, counts=True).splitlines())


def test_print_does_not_build_the_host_mirror(inputs):
    import yak_amd
    L = yak_amd.lib()
    h = L.yak_ch_restore(G.table_path("nb_k21", inputs[0]).encode())
    assert h
    try:
        L.yak_ch_tighten(h)
        before = L.yakamd_host_syncs()
        assert yak_amd.print_table(h, counts=True).count(b"\n") > 10000
        x, _ = yak_amd.kmers(h)
        assert len(x) > 10000 and L.yakamd_host_syncs() == before
        n = C.c_uint32()
        L.yak_ch_getseq.restype = C.c_void_p
        L.yak_ch_getseq.argtypes = [C.POINTER(yak_amd.ChT), C.c_int, C.POINTER(C.c_uint32)]
        C.CDLL(None).free(C.c_void_p(L.yak_ch_getseq(h, 0, C.byref(n))))
        assert L.yakamd_host_syncs() == before + 1                # the counter does see the mirror being built
    finally:
        L.yak_ch_destroy(h)


# ---- the binary listing against both getseqs ----
def lib_getseq(L, h, lo, hi):
    import yak_amd
    L.yak_ch_getseq.restype = C.POINTER(U.Knt)
    L.yak_ch_getseq.argtypes = [C.POINTER(yak_amd.ChT), C.c_int, C.POINTER(C.c_uint32)]
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    out = []
    for w in range(lo, hi):
        n = C.c_uint32()
        a = L.yak_ch_getseq(h, w, C.byref(n))
        out += [(a[j].x, a[j].c) for j in range(n.value)]
        free(C.cast(a, C.c_void_p))
    return out


def pairs_of(xc):
    return list(zip(xc[0].tolist(), xc[1].tolist()))


@pytest.mark.parametrize("k,pre", [(5, 10), (15, 10), (21, 12), (27, 10), (31, 12), (31, 10), (21, 10)])
def test_kmers_dev_equals_both_getseqs(k, pre, tmp_path, oracle):
    import yak_amd
    L, O = yak_amd.lib(), oracle.lib()
    fq, tab = str(tmp_path / "r.fq"), str(tmp_path / "t.yak")
    subprocess.check_call([SYN, "-n", "1500", "-l", "150", "-g", "9000", "-s", str(40 + k), "-o", fq])
    subprocess.run([CLI, "count", "-k%d" % k, "-p%d" % pre, "-o", tab, fq], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=T)
    h, ho = L.yak_ch_restore(tab.encode()), O.yko_ch_restore(tab.encode())
    assert h and ho
    try:
        P = 1 << pre
        empty = [w for w in range(P) if L.yakamd_kmers_dev(h, w, w + 1, None, None, 0) == 0]
        cuts = [0, 1, 7, P // 3, P - 1, P]
        ranges = [(0, P), (0, 1), (P - 1, P), (3, 3)] + list(zip(cuts[:-1], cuts[1:])) + ([(empty[0], empty[0] + 1)] if empty else [])
        if k == 5:
            assert empty, "k = 5 has at most 512 canonical k-mers: some of the 1024 sub-tables must be empty"
        for lo, hi in ranges:
            want = U.oracle_getseq(oracle, ho, lo, hi)
            assert pairs_of(yak_amd.kmers(h, lo, hi)) == want, (lo, hi)
        assert lib_getseq(L, h, 0, P) == U.oracle_getseq(oracle, ho)
        # a cap that is too small: the count needed comes back and nothing is written
        n = L.yakamd_kmers_dev(h, 0, P, None, None, 0)
        assert n == len(U.oracle_getseq(oracle, ho)) and n > 8
        dx, dc = L.yakamd_dev_alloc(n * 8), L.yakamd_dev_alloc(n * 2)
        fill = np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64)
        assert L.yakamd_memcpy_h2d(dx, fill.ctypes.data, n * 8) == 0 and L.yakamd_memcpy_h2d(dc, fill.ctypes.data, n * 2) == 0
        assert L.yakamd_kmers_dev(h, 0, P, dx, dc, n - 1) == n
        back = np.zeros(n, np.uint64)
        assert L.yakamd_memcpy_d2h(back.ctypes.data, dx, n * 8) == 0 and np.array_equal(back, fill)
        nb = L.yakamd_print_dev(h, 0, P, 1, None, 0)
        want_text = U.lines(U.oracle_getseq(oracle, ho), k, True)
        assert nb == len(want_text)
        dt = L.yakamd_dev_alloc(nb + 3)
        for shift in (0, 3):                                        # a text buffer at an odd address: the head / tail bytes of every tile
            assert L.yakamd_print_dev(h, 0, P, 1, dt + shift, nb - 1) == nb
            assert L.yakamd_print_dev(h, 0, P, 1, dt + shift, nb) == nb
            got = np.zeros(nb, np.uint8)
            assert L.yakamd_memcpy_d2h(got.ctypes.data, dt + shift, nb) == 0
            assert got.tobytes() == want_text
        for p in (dx, dc, dt):
            L.yakamd_dev_free(p)
        assert L.yakamd_kmers_dev(h, -1, 2, None, None, 0) == -1 and L.yakamd_kmers_dev(h, 0, P + 1, None, None, 0) == -1
    finally:
        L.yak_ch_destroy(h); O.yko_ch_destroy(ho)


# ---- tables that were never restored ----
def count_lib(L, fn, k, pre=10):
    import yak_amd
    co = yak_amd.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k, co.pre = k, pre
    h = L.yak_count(fn.encode(), C.byref(co), None)
    assert h, yak_amd._err()
    return h


def count_oracle(oracle, fn, k, pre=10):
    return oracle.lib().yko_count_file(fn.encode(), C.byref(oracle.copt(k=k, pre=pre)), None)


def test_counted_and_merged_tables_print_as_the_oracle_says(inputs, oracle):
    import yak_amd
    L, O = yak_amd.lib(), oracle.lib()
    _, p = inputs
    h, ho = count_lib(L, p["asm0.fa"], 21), count_oracle(oracle, p["asm0.fa"], 21)
    try:
        assert yak_amd.print_table(h, counts=True) == U.lines(U.oracle_getseq(oracle, ho), 21, True)   # the counting path's slot layout
        assert yak_amd.print_table(h, batch_bytes=1) == U.lines(U.oracle_getseq(oracle, ho), 21, False)
        n_first = len(U.oracle_getseq(oracle, ho))
        L.yak_ch_merge(h, count_lib(L, p["asm1.fa"], 21), 1, 1, 1, 0)
        O.yko_ch_merge(ho, count_oracle(oracle, p["asm1.fa"], 21), 1, 1, 0)
        want = U.lines(U.oracle_getseq(oracle, ho), 21, True)
        assert yak_amd.print_table(h, counts=True) == want and want.count(b"\n") > n_first > 50000   # the merge added k-mers
        assert pairs_of(yak_amd.kmers(h)) == U.oracle_getseq(oracle, ho)
    finally:
        L.yak_ch_destroy(h); O.yko_ch_destroy(ho)


def test_sharded_table_is_served(inputs, oracle, monkeypatch):
    import yak_amd
    L, O = yak_amd.lib(), oracle.lib()
    _, p = inputs
    whole = count_lib(L, p["asm0.fa"], 21)
    monkeypatch.setenv("YAKAMD_GPUS", "2"); monkeypatch.setenv("YAKAMD_GPU_LIST", "0,0")
    h = count_lib(L, p["asm0.fa"], 21)
    ho = count_oracle(oracle, p["asm0.fa"], 21)
    try:
        assert L.yakamd_last_sweeps() == 2
        got = yak_amd.print_table(h, counts=True)
        # a sub-table's layout depends on the stream of its own k-mers alone (count.c:129-143), which is the same in both prefix ranges' passes
        assert got == U.lines(U.oracle_getseq(oracle, ho), 21, True)
        assert sorted(got.splitlines()) == sorted(yak_amd.print_table(whole, counts=True).splitlines())
        assert yak_amd.print_table(h, batch_bytes=1) == U.lines(U.oracle_getseq(oracle, ho), 21, False)
        P = 1 << 10
        assert pairs_of(yak_amd.kmers(h, P // 2 - 3, P // 2 + 3)) == U.oracle_getseq(oracle, ho, P // 2 - 3, P // 2 + 3)   # across the shards
    finally:
        L.yak_ch_destroy(h); L.yak_ch_destroy(whole); O.yko_ch_destroy(ho)


# ---- k >= 32 ----
@pytest.mark.parametrize("name", G.REFUSED_TABLES)
def test_long_k_refused(name, tmp_path):
    import yak_amd
    L = yak_amd.lib()
    fn = os.path.join(GOLD, name + ".yak")
    for counts in (False, True):
        r = cli_print(fn, counts, check=False)
        assert r.returncode > 0 and r.returncode not in (134,) and r.stdout == b"" and b"below 32" in r.stderr
    h = L.yak_ch_restore(fn.encode())
    assert h
    try:
        P = 1 << h.contents.pre
        assert L.yakamd_kmers_dev(h, 0, P, None, None, 0) == -1 and b"below 32" in L.yakamd_last_error()
        assert L.yakamd_print_dev(h, 0, P, 0, None, 0) == -1
        o = yak_amd.PropT()
        L.yakamd_propt_init(C.byref(o))
        out = str(tmp_path / "o.txt")
        assert L.yakamd_print(C.byref(o), h, out.encode()) == -1 and not os.path.exists(out)
    finally:
        L.yak_ch_destroy(h)
    with pytest.raises(RuntimeError):
        yak_amd.print_kmers(fn)


# ---- cntasm, recount, subtract, isec ----
@pytest.mark.parametrize("group,name", [("cntasm", n) for n in G.CNTASM] + [("table_cmds", n) for n in G.TABLE_CMDS])
def test_table_command_equals_golden(group, name, gold, inputs, tmp_path):
    d, p = inputs
    steps = (G.CNTASM if group == "cntasm" else G.TABLE_CMDS)[name]
    got = G.run_case(CLI, steps, d, p, str(tmp_path / "out.yak"), timeout=T)
    assert G.expected(gold[group][name], got), (name, len(got))
    if group == "table_cmds":                                       # -o left out: the table goes to stdout
        assert G.run_case(CLI, steps, d, p, str(tmp_path / "unused.yak"), to_stdout=True, timeout=T) == got
    if os.path.exists(YAK_ON_AMD):
        assert G.run_case(YAK_ON_AMD, steps, d, p, str(tmp_path / "on_amd.yak"), timeout=T) == got


def test_cntasm_resume_overwrites_in_place(gold, inputs, tmp_path):
    d, p = inputs
    x = str(tmp_path / "x.yak")
    first = G.run_case(CLI, G.CNTASM["resume"][:1], d, p, x, timeout=T)
    assert open(x, "rb").read() == first
    second = G.run_case(CLI, G.CNTASM["resume"][1:], d, p, x, timeout=T)
    assert second != first and G.expected(gold["cntasm"]["resume"], second) and sorted(os.listdir(str(tmp_path))) == ["x.yak"]


@pytest.mark.parametrize("bad", [["-k32"], ["-k63"], ["-p9"], ["-k0"]])
def test_cntasm_refuses_bad_k_and_p(bad, inputs, tmp_path):
    _, p = inputs
    out = str(tmp_path / "o.yak")
    r = subprocess.run([CLI, "cntasm"] + bad + ["-o", out, p["asm0.fa"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    assert r.returncode > 0 and r.returncode != 134 and b"need 1 <= k < 32" in r.stderr and not os.path.exists(out)


def test_unreadable_tables_are_messages(inputs, tmp_path):
    _, p = inputs
    nope = str(tmp_path / "nope.yak")
    for args in (["recount", nope, p["digits_half.fa"]], ["subtract", nope, p["t0.yak"]], ["isec", p["t0.yak"], nope], ["print", nope]):
        r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
        assert r.returncode > 0 and r.returncode not in (134, 139) and r.stdout == b"" and b"yak-amd " + args[0].encode() in r.stderr, args


def test_usage_lists_thirteen_commands():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    names = [l.split()[1] for l in r.stderr.decode().splitlines() if l.startswith("    yak-amd ")]
    assert names == "count qv triobin trioeval inspect chkerr sexchr print cntasm recount subtract isec version".split()
    for n in names[7:12]:
        u = subprocess.run([CLI, n], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd " + n.encode())
    v = subprocess.run([CLI, "version"], stdout=subprocess.PIPE, timeout=60)
    assert v.returncode == 0 and v.stdout.strip()
