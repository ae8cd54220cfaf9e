"""`yak sexchr` on the device (k_lookup on the three SEXCHR loads + k_sc_reduce + yakamd_sexchr): byte-equal to the reference's
`sexchr -t1` on the stored fixtures at k = 21 and 41, the same bytes in any chunking, from stdin and from .gz; the tally export equal
to the Python restatement on random and adversarial arrays; tables of differing k refused with a message."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import chkerr_util as U
import gen_golden_sexchr as G
from test_gpu_triobin import Dev

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
NOKMER = 0xFF
KEY = "hap1.fa+hap2.fa"


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "sexchr.json")))


@pytest.fixture(scope="module")
def sc(tmp_path_factory, gold):
    d = tmp_path_factory.mktemp("sexchr")
    p = G.make_inputs(str(d))
    tabs = {}

    def tables(k):
        if k not in tabs:
            tabs[k] = []
            for t in G.TABLES:
                fn = str(d / ("%s_k%d.yak" % (t, k)))
                subprocess.run([CLI, "count", "-k%d" % k] + gold["count_args"] + ["-o", fn, p[t + ".fa"]], check=True,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                tabs[k].append(fn)
        return tabs[k]
    return d, p, tables


def cli(opts, tabs, h1, h2, check=True, **kw):
    r = subprocess.run([CLI, "sexchr"] + opts + list(tabs) + [h1, h2], check=check, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, **kw)
    return r if not check else r.stdout


@pytest.mark.parametrize("ks", ["k21", "k41"])
def test_cli_and_library_equal_golden(gold, sc, ks):
    import yak_amd
    _, p, tables = sc
    k = int(ks[1:])
    tabs = tables(k)
    assert [G.md5(t) for t in tabs] == gold["cases"][ks]["tables_md5"]
    want = gold["cases"][ks]["out"][KEY]
    got = cli([], tabs, p["hap1.fa"], p["hap2.fa"])
    assert G.T.expected(want, got), got.decode()[-2000:]
    assert yak_amd.sexchr(*tabs, p["hap1.fa"], p["hap2.fa"]) == got


@pytest.mark.parametrize("chunk", [1, 30000, 400000])
def test_chunks_do_not_show(gold, sc, chunk):
    import yak_amd
    _, p, tables = sc
    want = gold["cases"]["k41"]["out"][KEY]
    assert G.T.expected(want, yak_amd.sexchr(*tables(41), p["hap1.fa"], p["hap2.fa"], chunk=chunk))
    assert G.T.expected(gold["cases"]["k21"]["out"][KEY], cli(["-K", str(chunk)], tables(21), p["hap1.fa"], p["hap2.fa"]))


def test_stdin_and_gz(gold, sc):
    d, p, tables = sc
    gz = str(d / "hap2.fa.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(p["hap2.fa"], "rb").read())
    want = gold["cases"]["k21"]["out"][KEY]
    assert G.T.expected(want, cli([], tables(21), "-", gz, input=open(p["hap1.fa"], "rb").read()))


@pytest.mark.skipif(not os.path.exists(YAK_ON_AMD), reason="reference caller not built")
def test_reference_caller_on_library(sc):
    _, p, tables = sc
    for k in (21, 41):
        assert G.ref_sexchr(YAK_ON_AMD, tables(k), p["hap1.fa"], p["hap2.fa"]) == cli([], tables(k), p["hap1.fa"], p["hap2.fa"])


def test_tables_of_different_k_refused(sc):
    import yak_amd
    _, p, tables = sc
    t21, t41 = tables(21), tables(41)
    r = cli([], [t21[0], t41[1], t21[2]], p["hap1.fa"], p["hap2.fa"], check=False)
    assert r.returncode not in (0, -6, 134) and r.returncode > 0
    assert b"must agree" in r.stderr and r.stdout == b""
    with pytest.raises(ValueError):
        yak_amd.sexchr(t21[0], t21[1], t41[2], p["hap1.fa"], p["hap2.fa"])


def test_sharded_table_refused(sc, monkeypatch, tmp_path):
    import yak_amd
    L = yak_amd.lib()
    _, p, _ = sc
    monkeypatch.setenv("YAKAMD_GPUS", "2"); monkeypatch.setenv("YAKAMD_GPU_LIST", "0,0")
    co = yak_amd.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k = 21
    h = L.yak_count(p["chrX.fa"].encode(), C.byref(co), None)
    assert h, yak_amd._err()
    try:
        assert L.yakamd_last_sweeps() == 2
        o = yak_amd.ScoptT()
        L.yakamd_scopt_init(C.byref(o))
        assert L.yakamd_sexchr(C.byref(o), h, p["hap1.fa"].encode(), p["hap2.fa"].encode(), str(tmp_path / "o.txt").encode()) == -1
    finally:
        L.yak_ch_destroy(h)


# ---- the tally export against the restatement ----
def check_tally(seqs, lead=0):
    import yak_amd
    L = yak_amd.lib()
    off = np.zeros(len(seqs), np.uint64)
    buf, at = [np.full(lead, NOKMER, np.uint8)], lead
    for j, s in enumerate(seqs):
        off[j] = at
        buf.append(np.asarray(s, np.uint8)); buf.append(np.array([NOKMER], np.uint8))
        at += len(s) + 1
    flag = np.concatenate(buf)
    lens = np.array([len(s) for s in seqs], np.uint32)
    dev = Dev(L)
    try:
        d_f, d_off, d_len, d_cnt = dev.put(flag), dev.put(off), dev.put(lens), dev.empty(max(1, len(seqs)) * 32)
        assert L.yakamd_sexchr_reduce_dev(d_f, d_off, d_len, len(seqs), len(flag), d_cnt, None) == 0, yak_amd._err()
        got = dev.get(d_cnt, len(seqs) * 4, np.uint64).reshape(-1, 4)
    finally:
        dev.free()
    want = U.sexchr_tally(flag, off.tolist(), lens.tolist())
    assert np.array_equal(got, want)
    return int(got[:, 0].sum())


def flags(rng, n):
    return rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, NOKMER], np.uint8), size=n)


def test_tally_random():
    rng = np.random.default_rng(1)
    seqs = [flags(rng, int(n)) for n in rng.integers(0, 9000, 1500)]
    for lead in (0, 1, 15, 4095):
        assert check_tally(seqs, lead) > 1_000_000


def test_tally_many_empty_records_and_one_spanning_many_tiles():
    rng = np.random.default_rng(2)
    seqs = [np.zeros(0, np.uint8)] * 5000 + [flags(rng, 3_000_001)] + [flags(rng, int(n)) for n in rng.integers(0, 3, 20000)]
    check_tally(seqs)
    check_tally([np.ones(20 * 4096 + 3, np.uint8)] + [np.zeros(0, np.uint8)] * 3000 + [np.full(17, 2, np.uint8)])
