"""`yak-amd unitigs` on the device (k_graph_edges, k_graph_rank and k_graph_link of kern_graph.inc behind yakamd_graph_open, yakamd_graph_stats,
yakamd_graph_nodes_dev, yakamd_unitigs, the CLI and yak_amd.unitigs) against the restatement of DESIGN.md section 20 (tests/graph_util.py, held to
itself and to hand-derived cases by tests/test_graph.py), always on the dump of the very table that was probed: the tallies struct for struct, the
records one by one for tables of less than one step, of many workgroups, of more tiles than workgroups, with the directory in LDS and in global
memory, in any ranges of sub-tables; the size query, the two texts byte for byte in any batches, restored against resident tables, no host mirror
and the refusals."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import graph_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REC = np.dtype([("x", "<u8"), ("r", "<u8"), ("l", "<u8"), ("c", "<u4"), ("e", "<u4")])


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


class Tab:
    """a counted table, the .yak file of its dump and the restatement's view of that dump"""

    def __init__(self, ya, d, name, img, k, pre):
        self.t = ya.Table(k, pre, 4, 0)
        self.t.count_pass_host(1, img)
        self.k, self.pre, self.fn = k, pre, str(d / (name + ".yak"))
        open(self.fn, "wb").write(self.t.dump_bytes())
        kk, self.x, self.c = U.members(self.fn)
        assert kk == k
        self.want = {}

    def restated(self, min_cnt, walk=True):
        """(records, stats, unitigs) of the dump; walk = False: without the unitigs"""
        if min_cnt not in self.want:
            self.want[min_cnt] = U.graph(self.k, self.x, self.c, min_cnt) + (None,)
        recs, st, ug = self.want[min_cnt]
        if walk and ug is None:
            ug = U.unitigs(self.k, recs, min_cnt)
            self.want[min_cnt] = (recs, st, ug)
        return recs, st, ug


def mixed_k5():
    """one record of 160 random bases, 25 of 5 to 8, poly-A and (AC)n: at k = 5 about a third of all k-mers, sides of every degree from 0 to 4, a
    k-mer that is its own neighbour"""
    rng = random.Random(2)
    g = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    recs = [g(160)] + [g(rng.randint(5, 8)) for _ in range(25)] + ["A" * 12, "AC" * 8]
    return U.image([r.encode() for r in recs])


def restated_file(fn, min_cnt):
    k, x, c = U.members(fn)
    recs, st = U.graph(k, x, c, min_cnt)
    return k, recs, st, U.unitigs(k, recs, min_cnt)


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("graph")
    made = {}

    def get(name):
        if name not in made:
            kind, k, pre = name.split("_")
            k, pre = int(k[1:]), int(pre[1:])
            img = U.image(U.H.planted(k)) if kind == "planted" else mixed_k5() if kind == "mixed" else synth(2000, 150) if kind == "reads" else synth(16000, 150)
            made[name] = Tab(ya, d, name, img, k, pre)
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def check(tab, min_cnt, walk=True):
    recs, st, ug = tab.restated(min_cnt, walk)
    assert tab.t.graph_stats(min_cnt) == st
    got = tab.t.graph_nodes(min_cnt)
    assert len(got) == len(recs)
    assert got == recs
    return recs, st, ug


def unitigs_of(ya, h, min_cnt, out, stats=False, batch=None, threads=None):
    L = ya.lib()
    o = ya.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt, o.stats_only = min_cnt, int(stats)
    if batch is not None:
        o.batch_keys = batch
    if threads is not None:
        o.n_threads = threads
    if os.path.exists(out):
        os.remove(out)
    assert L.yakamd_unitigs(C.byref(o), h, out.encode()) == 0, ya._err()
    return open(out, "rb").read()


# planted k31 p10: less than one step of one workgroup's run; reads: ~50 k keys, many workgroups, the last tile of a sub-table partial; k21 p13: the
# directory in global memory, 8192 sub-tables of less than one tile; k5: sides of every degree from 0 to 4, a k-mer that is its own neighbour
@pytest.mark.parametrize("name", ["planted_k31_p10", "reads_k31_p10", "planted_k21_p13", "mixed_k5_p10"])
@pytest.mark.parametrize("min_cnt", [1, 3, 1023])
def test_tables_equal_restatement(ya, tabs, tmp_path, name, min_cnt):
    tab = tabs(name)
    recs, st, ug = check(tab, min_cnt)
    out = str(tmp_path / "o.txt")
    assert unitigs_of(ya, tab.t.h, min_cnt, out) == U.fasta_text(ug)
    assert unitigs_of(ya, tab.t.h, min_cnt, out, stats=True) == U.stats_text(tab.k, min_cnt, st, ug)
    if min_cnt == 1023:
        assert st["n_node"] == 0 and st["n_key"] == len(recs) > 0 and not ug and all(r[1] == r[2] == U.NONE and r[4] == 0 for r in recs)
        assert U.fasta_text(ug) == b""
    elif tab.k == 5 and min_cnt == 1:
        assert all(any(st["deg"][l][r] for r in range(5)) for l in range(5)) and all(any(st["deg"][l][r] for l in range(5)) for r in range(5))
        loops = 0
        for x, _, _, c, e in recs:                                # a k-mer that is its own neighbour has the bit like any other
            for s in (0, 1):
                for b in range(4):
                    z = int(U.extend(np.uint64(x), s, b, 5))
                    if min(z, int(U.H.revcomp(np.array([z], np.uint64), 5)[0])) == x:
                        loops += 1
                        assert e >> (4 * s + b) & 1
        assert loops > 0
    elif min_cnt == 1:
        assert st["deg"][1][1] > 1000 and st["n_linked_side"] > 1000


def test_cycle_and_lone_node_through_the_command(ya, tmp_path):
    """(AC)30 at k = 5 is two nodes linked into one cycle of 6 bases; A40 is one node, its own neighbour on both sides, and one open unitig"""
    for img, want in ((b"AC" * 30 + b"\n", b"\tLN:i:6\tKC:i:56\tkm:f:28.0\tCL:i:1\n"), (b"A" * 40 + b"\n", b">u0\tLN:i:5\tKC:i:36\tkm:f:36.0\tCL:i:0\nAAAAA\n")):
        tab = Tab(ya, tmp_path, "c%d" % len(img), img, 5, 10)
        try:
            recs, st, ug = check(tab, 1)
            text = unitigs_of(ya, tab.t.h, 1, str(tmp_path / "o.fa"))
            assert text == U.fasta_text(ug) and want in text and len(ug) == 1
            assert unitigs_of(ya, tab.t.h, 1, str(tmp_path / "o.txt"), stats=True) == U.stats_text(5, 1, st, ug)
        finally:
            tab.t.close()


def test_more_tiles_than_workgroups(ya, tabs, knob):
    """~350 k keys in 2^19 slots, 1024 tiles of 512 slots: as many as the default grid has workgroups at the most; with the grid held to 7 and to 300
    workgroups (the test switch YAKAMD_GRAPH_GRID) a workgroup walks on from tile to tile and sub-table to sub-table, in runs that do not divide
    the tiles evenly.  No result depends on the grid"""
    tab = tabs("big_k31_p10")
    assert len(tab.x) > 300000 and sum(tab.t.subtable(p)[0] for p in range(1 << tab.pre)) // 512 >= 1024
    check(tab, 1, walk=False)
    small = tabs("reads_k31_p10")
    for grid in (7, 300):
        knob("YAKAMD_GRAPH_GRID", grid)
        check(tab, 1, walk=False)
        check(small, 3)
        assert small.t.graph_nodes(1, 100, 611) == small.restated(1)[0][sum(small.t.subtable(p)[1] for p in range(100)):sum(small.t.subtable(p)[1] for p in range(611))]


def test_both_probe_schedules_give_the_same(ya, tabs, knob):
    """two rounds of four probes, or all eight requested together (the test switch YAKAMD_GRAPH_INFLIGHT)"""
    tab = tabs("reads_k31_p10")
    knob("YAKAMD_GRAPH_INFLIGHT", 8)
    check(tab, 1)
    check(tab, 3)


def test_ranges_of_sub_tables_glue_together(ya, tabs):
    L = ya.lib()
    for name, cuts in (("reads_k31_p10", [0, 1, 2, 300, 301, 777, 1024]), ("planted_k21_p13", [0, 4000, 4001, 8192]), ("mixed_k5_p10", [0, 512, 1024])):
        tab = tabs(name)
        recs, _, _ = tab.restated(1)
        kx, kc = ya.kmers(tab.t.h)                                # the records align with yakamd_kmers_dev: x and count are its output
        assert [int(v) for v in kx] == [r[0] for r in recs] and [int(v) for v in kc] == [r[3] for r in recs]
        glued = []
        for lo, hi in zip(cuts, cuts[1:]):
            part = tab.t.graph_nodes(1, lo, hi)
            assert len(part) == sum(tab.t.subtable(p)[1] for p in range(lo, hi))
            glued += part
        assert glued == recs                                       # links carry global listing indices in every range
        assert tab.t.graph_nodes(1, 5, 5) == []


def test_size_query_writes_nothing(ya, tabs):
    L = ya.lib()
    tab = tabs("reads_k31_p10")
    recs, _, _ = tab.restated(1)
    n = len(recs)
    g = L.yakamd_graph_open(tab.t.h, 1)
    assert g, ya._err()
    nb = n * 32 + 4096
    d = L.yakamd_dev_alloc(nb)
    assert d
    try:
        assert L.yakamd_graph_nodes_dev(g, 0, 1024, None, 0) == n == L.yakamd_graph_nodes_dev(g, 0, 1024, None, n)
        poison = bytes([0xA5]) * nb
        raw = C.create_string_buffer(nb)
        assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
        assert L.yakamd_graph_nodes_dev(g, 0, 1024, d, n - 1) == n and L.yakamd_graph_nodes_dev(g, 0, 1024, d, 0) == n
        assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
        assert L.yakamd_graph_nodes_dev(g, 0, 1024, d, n) == n
        assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
        assert raw.raw[n * 32:] == poison[n * 32:], "written past the last record"
        got = np.frombuffer(raw.raw[:n * 32], REC)
        assert [tuple(int(v) for v in r) for r in got] == recs
        # a middle range with more room than it needs: only its own records are written
        want = recs[sum(tab.t.subtable(p)[1] for p in range(100)):sum(tab.t.subtable(p)[1] for p in range(200))]
        assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
        assert L.yakamd_graph_nodes_dev(g, 100, 200, d, n) == len(want) > 0
        assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw[len(want) * 32:] == poison[len(want) * 32:]
        assert [tuple(int(v) for v in r) for r in np.frombuffer(raw.raw[:len(want) * 32], REC)] == want
        assert L.yakamd_graph_nodes_dev(g, 0, 1024, d + 8, n) == -1 and b"aligned" in L.yakamd_last_error()
        assert L.yakamd_graph_nodes_dev(g, 3, 2, d, n) == -1 and L.yakamd_graph_nodes_dev(g, 0, 1025, d, n) == -1
    finally:
        L.yakamd_dev_free(d)
        L.yakamd_graph_close(g)


@pytest.mark.parametrize("batch", [1000, 50000])
def test_batches_give_the_same_text(ya, tabs, knob, tmp_path, batch):
    tab = tabs("reads_k31_p10")
    assert batch == 50000 or len(tab.x) > 40 * batch
    out = str(tmp_path / "o.txt")
    for min_cnt in (1, 3):
        recs, st, ug = tab.restated(min_cnt)
        for stats, want in ((False, U.fasta_text(ug)), (True, U.stats_text(tab.k, min_cnt, st, ug))):
            assert unitigs_of(ya, tab.t.h, min_cnt, out, stats, batch=batch) == want
            assert unitigs_of(ya, tab.t.h, min_cnt, out, stats, threads=1) == want == unitigs_of(ya, tab.t.h, min_cnt, out, stats, threads=3)
            knob("YAKAMD_GRAPH_BATCH", batch)
            assert unitigs_of(ya, tab.t.h, min_cnt, out, stats) == want
            ya.lib().yakamd_test_reset()


def test_cli_and_python(ya, tabs, knob, tmp_path):
    tab = tabs("reads_k31_p10")
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))      # the command restores the file: the listing order is that table's
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
    finally:
        back.close()
    run = lambda a: subprocess.run([CLI, "unitigs"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    k, recs, st, ug = restated_file(f, 1)
    assert len(ug) > 100
    assert run([tab.fn]) == U.fasta_text(ug) == ya.unitigs(tab.fn) == ya.unitigs(tab.fn, batch_keys=1000, threads=2)
    assert run(["-s", "-t3", tab.fn]) == U.stats_text(k, 1, st, ug) == ya.unitigs(tab.fn, stats_only=True, batch_keys=50000)
    assert subprocess.run([CLI, "-X", "YAKAMD_GRAPH_BATCH=1000", "unitigs", tab.fn], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout == U.fasta_text(ug)
    knob("YAKAMD_GRAPH_BATCH", 1000)
    assert ya.unitigs(tab.fn) == U.fasta_text(ug)
    ya.lib().yakamd_test_reset()
    k, recs3, st3, ug3 = restated_file(f, 3)
    out = str(tmp_path / "o.fa")
    assert run(["-c3", "-o", out, tab.fn]) == b"" and open(out, "rb").read() == U.fasta_text(ug3) == ya.unitigs(tab.fn, min_cnt=3)
    assert run(["-c3", "-s", tab.fn]) == U.stats_text(k, 3, st3, ug3)
    assert run(["-c1023", tab.fn]) == b"" and run(["-c1023", "-s", tab.fn]) == U.stats_text(k, 1023, dict(st, n_node=0, n_arc=0, n_linked_side=0, deg=[[0] * 5] * 5), [])
    r = subprocess.run([CLI, "unitigs"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"usage: yak-amd unitigs" in r.stderr and r.stdout == b""
    usage = subprocess.run([CLI], stderr=subprocess.PIPE).stderr.decode()
    assert "      yak-amd unitigs" in usage.split("beyond the reference")[1]
    for a in (["-c", "0", "-o", out + "2", tab.fn], ["-c1024", "-o", out + "2", tab.fn], ["-t0", "-o", out + "2", tab.fn]):
        r = subprocess.run([CLI, "unitigs"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out + "2"), a


def test_restored_and_resident_tables_agree(ya, tmp_path):
    """the table yak_count() returns and the table restored from its file hold the same k-mers: the same tallies and the same unitigs as sets (the
    listing order, and with it the order and orientation of the output, is each table's own)"""
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
            assert res.graph_stats(1) == back.graph_stats(1)
            sets = []
            for i, t in enumerate((res, back)):                       # each against the restatement in its own table's order
                f = str(tmp_path / ("own%d.yak" % i))
                open(f, "wb").write(t.dump_bytes())
                k, recs, st, ug = restated_file(f, 1)
                assert t.graph_nodes(1) == recs
                text = unitigs_of(ya, t.h, 1, str(tmp_path / "o.fa"))
                assert text == U.fasta_text(ug)
                sets.append(sorted(U.canon(l.decode()) for l in text.split(b"\n")[1::2]))
            assert sets[0] == sets[1] and len(sets[0]) > 50
        finally:
            back.close()
    finally:
        res.close()


def test_no_host_mirror(ya, tabs, tmp_path):
    L = ya.lib()
    tab = tabs("planted_k31_p10")
    back = ya.Table(ptr=L.yak_ch_restore(tab.fn.encode()))
    try:
        before = L.yakamd_host_syncs()
        st = back.graph_stats(1)
        recs = back.graph_nodes(1)
        text = unitigs_of(ya, back.h, 1, str(tmp_path / "o.fa"))
        unitigs_of(ya, back.h, 1, str(tmp_path / "o.txt"), stats=True)
        assert L.yakamd_host_syncs() == before
        assert st == tab.restated(1)[1] and sorted(r[0] for r in recs) == sorted(r[0] for r in tab.restated(1)[0]) and text
        L.yak_ch_get.restype = C.c_int
        L.yak_ch_get(back.h, 12345)
        assert L.yakamd_host_syncs() == before + 1                # the counter does see a mirror being built
    finally:
        back.close()


# ---- refusals: each its own message, before any output ----
def refused(ya, h, out, capfd, what, min_cnt=1):
    L = ya.lib()
    o = ya.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt = min_cnt
    assert L.yakamd_graph_open(h, min_cnt) is None and what.encode() in L.yakamd_last_error(), L.yakamd_last_error()
    capfd.readouterr()
    assert L.yakamd_unitigs(C.byref(o), h, out.encode()) == -1
    assert what in capfd.readouterr().err and what.encode() in L.yakamd_last_error()
    assert not os.path.exists(out), "a refused call created its output"


def test_refusals(ya, synth, knob, capfd, tmp_path):
    L = ya.lib()
    out = str(tmp_path / "o.txt")
    buf = synth(300, 150, 2500, s=5)
    refused(ya, None, out, capfd, "not an engine table")
    for k, what in ((30, "even"), (41, "below 32")):
        t = ya.Table(k, 10, 4, 0)
        try:
            t.count_pass_host(1, buf)
            refused(ya, t.h, out, capfd, what)
        finally:
            t.close()
    t = ya.Table(21, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        refused(ya, t.h, out, capfd, "min_cnt 0", min_cnt=0)
        refused(ya, t.h, out, capfd, "min_cnt 1024", min_cnt=1024)
        g = L.yakamd_graph_open(t.h, 1)
        assert g, ya._err()
        try:
            st = ya.GstatT()
            assert L.yakamd_graph_stats(g, C.byref(st)) == 0 and st.n_node > 0
            assert L.yakamd_pass_begin(t.h, 0) == 0
            refused(ya, t.h, out, capfd, "open pass")
            assert L.yakamd_graph_stats(g, C.byref(st)) == -1 and b"open pass" in L.yakamd_last_error()     # refused again at each later call
            assert L.yakamd_graph_nodes_dev(g, 0, 1024, None, 0) == -1 and b"open pass" in L.yakamd_last_error()
            assert L.yakamd_pass_end(t.h) >= 0
            assert L.yakamd_graph_stats(g, C.byref(st)) == 0
        finally:
            L.yakamd_graph_close(g)
        assert t.graph_stats(1)["n_node"] == st.n_node > 0            # and the table serves again
        before = t.dump_bytes()
        t.graph_nodes(1)
        assert t.dump_bytes() == before                               # the table is not modified
    finally:
        t.close()
    fa = str(tmp_path / "r.fa")
    open(fa, "wb").write(U.fasta(buf.split(b"\n")[:-1]))
    knob("YAKAMD_GPUS", 2)
    knob("YAKAMD_GPU_LIST", "0,0")
    co = ya.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k = 21
    h = L.yak_count(fa.encode(), C.byref(co), None)
    assert h, ya._err()
    try:
        assert L.yakamd_last_sweeps() == 2
        refused(ya, h, out, capfd, "sharded over prefix ranges")
    finally:
        L.yak_ch_destroy(h)
