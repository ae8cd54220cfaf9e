"""The walk of `yak-amd unitigs -g` on the device (the kernels of yak_amd/walk/walk.hip behind yakamd_uwalk_open, the three _dev getters,
yakamd_unitigs_dev, the CLI and yak_amd.walk) against the restatement of tests/walk_util.py (held to hand-derived cases and to the sequential model
of the kernels by tests/test_walk.py), always on the dump of the very table that was walked: the tallies, the node -> unitig map, the descriptors
and the bases element by element; both texts byte for byte against the restatement and against yakamd_unitigs on the same table; one unitig of
about 12 and a chain across every sub-table of about 17 doubling rounds, more unitigs than one tile of the scan, a table without a node, cycles
alone and beside open unitigs; the size queries, restored against resident tables, the refusals, and a launch of every kernel of the library."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import graph_util as U
import walk_util as W
from test_gpu_graph import CLI, Tab, mixed_k5, restated_file, unitigs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the walk has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def yw(ya):
    import yak_amd.walk
    yak_amd.walk.lib()
    return yak_amd.walk


def genome(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


SHAPES = {
    "genome3000_k31_p10": lambda synth: U.image([genome(3000, 31)]),
    "genome70000_k21_p13": lambda synth: U.image([genome(70000, 70)]),
    "reads_k31_p10": lambda synth: synth(2000, 150),
    "mixed_k5_p10": lambda synth: mixed_k5(),
    "ac8_k5_p10": lambda synth: U.image([b"AC" * 8]),
    # two random records, (AC)20 and (ACG)14: at k = 31 a cycle of two and a cycle of three nodes whose listing indices lie among those of two chains
    "cycles_k31_p10": lambda synth: U.image([genome(3000, 31), b"AC" * 20, genome(500, 5), b"ACG" * 14]),
}


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("walk")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](synth), int(k[1:]), int(pre[1:]))
            tab.walk_want = {}
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def want_of(tab, min_cnt):
    """(records, graph tallies, unitigs, (map, desc, bases), stats) of the dump, computed once"""
    if min_cnt not in tab.walk_want:
        recs, st, ug = tab.restated(min_cnt)
        tab.walk_want[min_cnt] = (recs, st, ug, W.restate(tab.k, recs, min_cnt, ug), W.stats(tab.k, recs, min_cnt, ug))
    return tab.walk_want[min_cnt]


def unitigs_dev_of(ya, yw, h, min_cnt, out, stats=False):
    o = ya.UgoptT()
    ya.lib().yakamd_ugopt_init(C.byref(o))
    o.min_cnt, o.stats_only, o.n_threads, o.batch_keys = min_cnt, int(stats), 0, 0     # the last two are ignored
    if os.path.exists(out):
        os.remove(out)
    assert yw.lib().yakamd_unitigs_dev(C.byref(o), h, out.encode()) == 0, yw._err()
    return open(out, "rb").read()


def check(ya, yw, tab, min_cnt, tmp_path):
    recs, st, ug, (amap, desc, bases), stats = want_of(tab, min_cnt)
    with yw.Walk(tab.t, min_cnt) as w:
        got = w.stats()
        print("stats", got)
        assert {f: got[f] for f in stats} == stats
        assert got["host_nodes"] <= W.cycle_nodes(ug) and 1 <= got["rounds"] <= 64
        assert w.gstat() == st
        m, d, b = w.map(), w.desc(), w.bases()
        assert len(m) == len(amap) and len(d) == len(desc) and len(b) == len(bases)
        want_m = np.array(amap, np.uint64).reshape(-1, 2)
        assert np.array_equal(m["unitig"], want_m[:, 0]) and np.array_equal(m["at"], want_m[:, 1])
        want_d = np.array(desc, np.uint64).reshape(-1, 4)
        for i, f in enumerate(("off", "n_node", "kc", "first")):
            assert np.array_equal(d[f], want_d[:, i]), f
        assert b.tobytes() == bases
    out = str(tmp_path / "o.txt")
    fa = unitigs_dev_of(ya, yw, tab.t.h, min_cnt, out)
    assert fa == U.fasta_text(ug) and fa == unitigs_of(ya, tab.t.h, min_cnt, out)
    tx = unitigs_dev_of(ya, yw, tab.t.h, min_cnt, out, stats=True)
    assert tx == U.stats_text(tab.k, min_cnt, st, ug) and tx == unitigs_of(ya, tab.t.h, min_cnt, out, stats=True)
    return got, ug


def test_one_unitig_of_a_genome(ya, yw, tabs, tmp_path):
    """2970 nodes in one chain: a state L links from its terminal finishes in round floor(log2 L) + 1, one more round ends the ranking"""
    got, ug = check(ya, yw, tabs("genome3000_k31_p10"), 1, tmp_path)
    assert len(ug) == 1 and got["n_open"] == 1 and got["n_node"] == 2970 and got["rounds"] == (2969).bit_length() + 1 == 13 and got["host_nodes"] == 0


def test_a_chain_across_every_sub_table(ya, yw, tabs, tmp_path):
    tab = tabs("genome70000_k21_p13")
    got, ug = check(ya, yw, tab, 1, tmp_path)
    assert len(ug) == 1 and got["n_node"] == 69980 and got["rounds"] == (69979).bit_length() + 1 == 18
    assert sum(1 for p in range(1 << 13) if tab.t.subtable(p)[1] >= 1) > 8000


@pytest.mark.parametrize("min_cnt", [1, 3, 1023])
def test_reads(ya, yw, tabs, tmp_path, min_cnt):
    """with the error k-mers (min_cnt 1) many single nodes and more unitigs than one tile of the scan; at 1023 the table without a node"""
    got, ug = check(ya, yw, tabs("reads_k31_p10"), min_cnt, tmp_path)
    if min_cnt == 1:
        assert got["n_open"] > 2 * 1024 and sum(1 for u in ug if u[1] == 1) > 100
    if min_cnt == 1023:
        assert got["n_key"] > 1000 and got["n_node"] == got["n_open"] == got["sum_len"] == got["n50"] == 0 and got["rounds"] == 1


def test_every_degree_at_k5(ya, yw, tabs, tmp_path):
    got, ug = check(ya, yw, tabs("mixed_k5_p10"), 1, tmp_path)
    assert got["n_open"] > 100
    check(ya, yw, tabs("mixed_k5_p10"), 2, tmp_path)


def test_nothing_but_a_cycle(ya, yw, tabs, tmp_path):
    got, ug = check(ya, yw, tabs("ac8_k5_p10"), 1, tmp_path)
    assert (got["n_open"], got["n_cycle"], got["n_node"], got["sum_len"], got["host_nodes"]) == (0, 1, 2, 6, 2)


def test_cycles_beside_open_unitigs(ya, yw, tabs, tmp_path):
    """the compaction of the cycles' records picks 5 of ~3450 keys by the scan, their descriptors and bases go behind those of the open unitigs
    (j0 = n_open, off0 = the open unitigs' bases), and k_uw_emit leaves the map entries of the cycle nodes to k_uw_cyc_scatter"""
    tab = tabs("cycles_k31_p10")
    got, ug = check(ya, yw, tab, 1, tmp_path)
    assert got["n_open"] == 2 and got["n_cycle"] == 2 and 0 < got["host_nodes"] == W.cycle_nodes(ug) == 5 < got["n_node"]
    recs, st, ug, (amap, desc, bases), stats = want_of(tab, 1)
    on_cycle = [v for v, m in enumerate(amap) if m[0] >= got["n_open"]]
    assert len(on_cycle) == 5 and on_cycle != list(range(5)) and on_cycle[0] > 0 and on_cycle[-1] < len(amap) - 1      # among the open nodes
    assert sorted(d[1] for d in desc[:2]) == [470, 2970] and sorted(d[1] for d in desc[2:]) == [2, 3] and all(d[3] & 1 for d in desc[2:])
    assert desc[2][0] == 3000 + 500 and desc[3][0] == 3500 + desc[2][1] + 30


def test_size_queries_write_nothing(ya, yw, tabs):
    L = ya.lib()
    tab = tabs("reads_k31_p10")
    with yw.Walk(tab.t, 1) as w:
        st = w.stats()
        for getter, n, each in ((w.L.yakamd_uwalk_map_dev, st["n_key"], 16), (w.L.yakamd_uwalk_desc_dev, st["n_open"] + st["n_cycle"], 32),
                                (w.L.yakamd_uwalk_bases_dev, st["sum_len"], 1)):
            assert n > 0
            nb = n * each + 4096
            d = L.yakamd_dev_alloc(nb)
            assert d
            try:
                poison = bytes([0xA5]) * nb
                raw = C.create_string_buffer(nb)
                assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
                assert getter(w.w, None, 0) == n == getter(w.w, None, n) == getter(w.w, d, n - 1) == getter(w.w, d, 0)
                assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
                assert getter(w.w, d, n + 7) == n
                assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
                assert raw.raw[n * each:] == poison[n * each:], "written past the last entry"
                assert raw.raw[:n * each] != poison[:n * each]
                if each > 1:
                    assert getter(w.w, d + 8, n) == -1 and b"aligned" in w.L.yakamd_walk_last_error()
            finally:
                L.yakamd_dev_free(d)
    assert yw.lib().yakamd_uwalk_map_dev(None, None, 0) == -1 and yw.lib().yakamd_uwalk_stats(None, None) == -1
    yw.lib().yakamd_uwalk_close(None)


def test_cli_and_python(ya, yw, tabs, tmp_path):
    tab = tabs("reads_k31_p10")
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))      # the command restores the file: the listing order is that table's
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
    finally:
        back.close()
    run = lambda a: subprocess.run([CLI, "unitigs"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    for min_cnt in (1, 3):
        k, recs, st, ug = restated_file(f, min_cnt)
        c = ["-c%d" % min_cnt]
        assert run(c + ["-g", tab.fn]) == U.fasta_text(ug) == yw.unitigs_dev(tab.fn, min_cnt=min_cnt) == run(c + [tab.fn])
        assert run(c + ["-g", "-s", tab.fn]) == U.stats_text(k, min_cnt, st, ug) == yw.unitigs_dev(tab.fn, min_cnt=min_cnt, stats_only=True) == run(c + ["-s", tab.fn])
    out = str(tmp_path / "o.fa")
    assert run(["-g", "-c3", "-o", out, tab.fn]) == b"" and open(out, "rb").read() == U.fasta_text(ug)
    assert run(["-g", "-c1023", tab.fn]) == b"" and run(["-g", "-c1023", "-s", tab.fn]) == run(["-c1023", "-s", tab.fn])
    for a in (["-g", "-c", "0", "-o", out + "2", tab.fn], ["-g", "-c1024", "-o", out + "2", tab.fn]):
        r = subprocess.run([CLI, "unitigs"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out + "2"), a
    r = subprocess.run([CLI, "unitigs", "-g", "-o", out + "2", tab.fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, YAKAMD_WALK_MAX_BYTES="1"))
    assert r.returncode == 3 and b"bytes of device memory are needed" in r.stderr and not os.path.exists(out + "2")


def test_restored_and_resident_tables_agree(ya, yw, tmp_path):
    """the table yak_count() returns and the table restored from its file: each walk against the restatement in its own table's order, and the same
    unitigs as sets"""
    L = ya.lib()
    fa = str(tmp_path / "p.fa")
    open(fa, "wb").write(U.fasta(U.H.planted(31)))
    co = ya.CoptT()
    L.yak_copt_init(C.byref(co))
    h = L.yak_count(fa.encode(), C.byref(co), None)
    assert h, ya._err()
    res = ya.Table(ptr=h)
    fn = str(tmp_path / "p.yak")
    try:
        assert L.yak_ch_dump(h, fn.encode()) == 0
        back = ya.Table(ptr=L.yak_ch_restore(fn.encode()))
        try:
            sets = []
            for i, t in enumerate((res, back)):
                f = str(tmp_path / ("own%d.yak" % i))
                open(f, "wb").write(t.dump_bytes())
                k, recs, st, ug = restated_file(f, 1)
                amap, desc, bases = W.restate(k, recs, 1, ug)
                with yw.Walk(t, 1) as w:
                    assert [tuple(int(v) for v in e) for e in w.map()] == amap and [tuple(int(v) for v in e) for e in w.desc()] == desc and w.bases().tobytes() == bases
                text = unitigs_dev_of(ya, yw, t.h, 1, str(tmp_path / "o.fa"))
                assert text == U.fasta_text(ug)
                sets.append(sorted(U.canon(l.decode()) for l in text.split(b"\n")[1::2]))
            assert sets[0] == sets[1] and len(sets[0]) > 50
        finally:
            back.close()
    finally:
        res.close()


# ---- refusals: each with its message, before any output ----
def refused(ya, yw, h, out, what, min_cnt=1):
    WL = yw.lib()
    o = ya.UgoptT()
    ya.lib().yakamd_ugopt_init(C.byref(o))
    o.min_cnt = min_cnt
    assert WL.yakamd_uwalk_open(h, min_cnt) is None and what.encode() in WL.yakamd_walk_last_error(), WL.yakamd_walk_last_error()
    assert WL.yakamd_unitigs_dev(C.byref(o), h, out.encode()) == -1 and what.encode() in WL.yakamd_walk_last_error()
    assert not os.path.exists(out), "a refused call created its output"


def test_refusals(ya, yw, synth, monkeypatch, tmp_path):
    L = ya.lib()
    out = str(tmp_path / "o.txt")
    buf = synth(300, 150, 2500, s=5)
    refused(ya, yw, None, out, "not an engine table")
    for k, what in ((30, "even"), (32, "k = 32"), (41, "below 32")):
        t = ya.Table(k, 10, 4, 0)
        try:
            t.count_pass_host(1, buf)
            refused(ya, yw, t.h, out, what)
        finally:
            t.close()
    t = ya.Table(21, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        refused(ya, yw, t.h, out, "min_cnt 0", min_cnt=0)
        refused(ya, yw, t.h, out, "min_cnt 1024", min_cnt=1024)
        assert L.yakamd_pass_begin(t.h, 0) == 0
        refused(ya, yw, t.h, out, "open pass")
        assert L.yakamd_pass_end(t.h) >= 0
        monkeypatch.setenv("YAKAMD_WALK_MAX_BYTES", "1")
        refused(ya, yw, t.h, out, "bytes of device memory are needed")
        need = int(re.search(rb"(\d+) bytes of device memory are needed", yw.lib().yakamd_walk_last_error()).group(1))
        n_key = t.graph_stats(1)["n_key"]
        assert need > 120 * n_key > 0                                 # records, two pair buffers, indices and the map: 120 bytes per stored key, and more
        monkeypatch.setenv("YAKAMD_WALK_MAX_BYTES", str(need - 1))
        refused(ya, yw, t.h, out, "bytes of device memory are needed")
        monkeypatch.setenv("YAKAMD_WALK_MAX_BYTES", str(need))
        before = t.dump_bytes()
        with yw.Walk(t, 1) as w:                                       # exactly what it asked for is enough, and the table serves again
            assert w.stats()["n_key"] == n_key
        assert t.dump_bytes() == before                               # the table is not modified
    finally:
        t.close()


def test_every_kernel_is_launched(ya, yw, tabs):
    """the k5 table and the 70 000-base chain, and the cycles beside open unitigs and (AC)8 for the kernels of the cycles (the k5 table's AC
    k-mers have other neighbours): no instantiation in the library's tally without a test that launches it"""
    names = set(yw.tally())
    assert {"k_uw_init", "k_uw_jump", "k_uw_decide", "k_uw_emit", "k_uw_tile_scan", "k_uw_cyc_gather"} <= names and not [n for n in names if n.startswith("event:")]
    yw.lib().yakamd_walk_tally_reset()
    assert not any(yw.tally().values())
    for name in ("mixed_k5_p10", "genome70000_k21_p13", "cycles_k31_p10", "ac8_k5_p10"):
        with yw.Walk(tabs(name).t, 1) as w:
            rounds = w.stats()["rounds"]
    got = yw.tally()
    assert all(v > 0 for v in got.values()), got
    assert got["k_uw_init"] == 4 and got["k_uw_jump"] >= rounds + 3 and got["k_uw_cyc_scatter"] == got["k_uw_cyc_gather"] == 2
