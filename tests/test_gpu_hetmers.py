"""`yak-amd hetmers` on the device (k_hetmer of kern_hetmer.inc behind yakamd_hetmers_dev, yakamd_hetmer_pairs_dev, yakamd_hetmers, the CLI and
yak_amd.hetmers) against the restatement of DESIGN.md section 17 (tests/hetmer_util.py, held to itself and to hand-derived numbers by
tests/test_hetmers.py), always on the dump of the very table that was probed: the histogram, the group counts and the ordered pair list for tables
of one step, of many workgroups, of several steps per workgroup, with the directory and the offsets in LDS and in global memory, in any ranges;
the size query, restored against resident tables, no host mirror, the refusals and the command's text byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import hetmer_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")


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
        self.k, self.fn = k, str(d / (name + ".yak"))
        open(self.fn, "wb").write(self.t.dump_bytes())
        kk, self.x, self.c = U.members(self.fn)
        assert kk == k
        self.want = {}

    def restated(self, min_cnt):
        if min_cnt not in self.want:
            self.want[min_cnt] = U.hetmers(self.k, self.x, self.c, min_cnt)
        return self.want[min_cnt]


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("hetmers")
    made = {}

    def get(name):
        if name not in made:
            kind, k, pre = name.split("_")
            k, pre = int(k[1:]), int(pre[1:])
            img = U.image(U.planted(k)) if kind == "planted" else synth(2000, 150) if kind == "reads" else synth(16000, 150)
            made[name] = Tab(ya, d, name, img, k, pre)
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def check(tab, min_cnt):
    J, g, pairs = tab.restated(min_cnt)
    gotJ, gotg = tab.t.hetmers(min_cnt)
    assert gotg == g, (gotg, g)
    assert gotJ == J
    assert tab.t.hetmer_pairs(min_cnt) == pairs
    return J, g, pairs


# planted k31 p10: less than one step of one workgroup; reads: ~50 k keys, many workgroups, the last step partial; k21 p13: the directory and (8192
# sub-tables) the key offsets in global memory; k5: dense, groups of four, palindromic flanks of two bases
@pytest.mark.parametrize("name", ["planted_k31_p10", "reads_k31_p10", "planted_k21_p13", "planted_k5_p10"])
@pytest.mark.parametrize("min_cnt", [1, 3, 1023])
def test_tables_equal_restatement(tabs, name, min_cnt):
    tab = tabs(name)
    J, g, pairs = check(tab, min_cnt)
    if min_cnt == 1023:
        assert g == [0] * 5 and not J and not pairs
    elif name.startswith("planted") and tab.k in U.EXPECT:
        want = (U.EXPECT if min_cnt == 1 else U.EXPECT_MIN3)[tab.k]
        assert g == want["n_group"] and J == want["J"]
    elif min_cnt == 1:
        assert (g[4] > 50) if tab.k == 5 else (g[2] > 100 and len(tab.x) % 512 != 0)


def test_several_steps_per_workgroup(tabs):
    """more tiles than the grid has workgroups (two per CU, 512 keys a tile): a workgroup's lanes walk on through the sub-tables from step to step"""
    tab = tabs("big_k31_p10")
    assert len(tab.x) > 300000
    J, g, pairs = check(tab, 1)
    assert len(pairs) > 1000
    check(tab, 2)


@pytest.mark.parametrize("batch", [1000, 50000])
def test_ranges_give_the_same(ya, tabs, knob, batch):
    tab = tabs("reads_k31_p10")
    assert batch == 50000 or len(tab.x) > 40 * batch
    one = ya.hetmers(tab.fn, pairs=True)
    knob("YAKAMD_HETMER_BATCH", batch)
    check(tab, 1)
    check(tab, 3)
    assert ya.hetmers(tab.fn, pairs=True) == one
    ya.lib().yakamd_test_reset()
    assert ya.hetmers(tab.fn, pairs=True, batch_keys=batch) == one      # the option, without the switch


def test_pair_list_size_query_writes_nothing(ya, tabs):
    L = ya.lib()
    tab = tabs("reads_k31_p10")
    _, _, pairs = tab.restated(1)
    n = len(pairs)
    assert n > 100
    assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, None, 0) == n
    assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, None, n) == n
    nb = n * 24 + 64
    d = L.yakamd_dev_alloc(nb)
    assert d
    try:
        poison = bytes([0xA5]) * nb
        raw = C.create_string_buffer(nb)
        assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
        assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, d, n - 1) == n
        assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, d, 0) == n
        assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
        assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, d, n) == n
        assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
        assert raw.raw[n * 24:] == poison[n * 24:], "written past the last record"
        got = np.frombuffer(raw.raw[:n * 24], np.dtype([("x", "<u8"), ("y", "<u8"), ("cx", "<u4"), ("cy", "<u4")]))
        assert [tuple(int(v) for v in r) for r in got] == pairs
        assert L.yakamd_hetmer_pairs_dev(tab.t.h, 1, d + 4, n) == -1 and b"aligned" in L.yakamd_last_error()
    finally:
        L.yakamd_dev_free(d)


def test_restored_and_resident_tables_agree(ya, tabs, tmp_path):
    """the table yak_count() returns and the table restored from its file: the same k-mers, so the same histogram, groups and set of pairs
    (the listing order is each table's own)"""
    L = ya.lib()
    fa = str(tmp_path / "p.fa")
    open(fa, "wb").write(U.fasta(U.planted(31)))
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
            a, b = res.hetmers(1), back.hetmers(1)
            assert a == b and a[1] == U.EXPECT[31]["n_group"] and a[0] == U.EXPECT[31]["J"]
            pa, pb = res.hetmer_pairs(1), back.hetmer_pairs(1)
            assert sorted(pa) == sorted(pb) and len(pa) == 28
            for t, p in ((res, pa), (back, pb)):                       # each in its own table's order
                f = str(tmp_path / "own.yak")
                open(f, "wb").write(t.dump_bytes())
                assert U.hetmers(*U.members(f), 1)[2] == p
        finally:
            back.close()
    finally:
        res.close()


def test_no_host_mirror(ya, tabs, tmp_path):
    """across the three calls, on a table restored before (yak_ch_init, behind the restore, takes the empty table's mirror once)"""
    L = ya.lib()
    tab = tabs("planted_k31_p10")
    back = ya.Table(ptr=L.yak_ch_restore(tab.fn.encode()))
    try:
        o = ya.HmoptT()
        L.yakamd_hmopt_init(C.byref(o))
        o.print_pairs = 1
        out = str(tmp_path / "o.txt")
        before = L.yakamd_host_syncs()
        J, g = back.hetmers(1)
        pairs = back.hetmer_pairs(1)
        assert L.yakamd_hetmers(C.byref(o), back.h, out.encode()) == 0, ya._err()
        assert L.yakamd_host_syncs() == before
        assert open(out, "rb").read() == U.text(31, 1, J, g, pairs)
        assert (J, g) == tab.restated(1)[:2] and sorted(pairs) == sorted(tab.restated(1)[2])
        L.yak_ch_get.restype = C.c_int
        L.yak_ch_get(back.h, 12345)
        assert L.yakamd_host_syncs() == before + 1                # the counter does see a mirror being built
    finally:
        back.close()


# ---- refusals: each its own message, before any output ----
def refused(ya, h, out, capfd, what, min_cnt=1):
    L = ya.lib()
    o = ya.HmoptT()
    L.yakamd_hmopt_init(C.byref(o))
    o.min_cnt = min_cnt
    d = L.yakamd_dev_alloc(64)
    try:
        for call in (lambda: L.yakamd_hetmers_dev(h, min_cnt, d, d, None), lambda: L.yakamd_hetmer_pairs_dev(h, min_cnt, None, 0)):
            assert call() == -1 and what.encode() in L.yakamd_last_error(), L.yakamd_last_error()
    finally:
        L.yakamd_dev_free(d)
    capfd.readouterr()
    assert L.yakamd_hetmers(C.byref(o), h, out.encode()) == -1
    assert what in capfd.readouterr().err and what.encode() in L.yakamd_last_error()
    assert not os.path.exists(out), "a refused call created its output"


def test_refusals(ya, tabs, synth, knob, capfd, tmp_path):
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
        assert L.yakamd_pass_begin(t.h, 0) == 0
        refused(ya, t.h, out, capfd, "open pass")
        assert L.yakamd_pass_end(t.h) >= 0
        assert t.hetmers(1)[1][1] > 0                              # and served again after the pass
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


def test_cli(ya, tabs, tmp_path):
    tab = tabs("reads_k31_p10")
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))      # the command restores the file: the listing order is that table's
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
        k, x, c = U.members(f)
    finally:
        back.close()
    run = lambda a: subprocess.run([CLI, "hetmers"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    J, g, pairs = U.hetmers(k, x, c, 1)
    assert run([tab.fn]) == U.text(k, 1, J, g) == ya.hetmers(tab.fn)
    J3, g3, pairs3 = U.hetmers(k, x, c, 3)
    out = str(tmp_path / "o.txt")
    assert run(["-p", "-c3", "-o", out, tab.fn]) == b"" and open(out, "rb").read() == U.text(k, 3, J3, g3, pairs3)
    assert pairs and run(["-p", tab.fn]) == U.text(k, 1, J, g, pairs)
    r = subprocess.run([CLI, "hetmers"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"usage: yak-amd hetmers" in r.stderr and r.stdout == b""
    usage = subprocess.run([CLI], stderr=subprocess.PIPE).stderr.decode()
    assert "beyond the reference" in usage and "yak-amd hetmers" in usage.split("beyond the reference")[1]
    even = str(tmp_path / "k30.yak")
    t = ya.Table(30, 10, 4, 0)
    try:
        t.count_pass_host(1, U.image(U.planted(31)))
        open(even, "wb").write(t.dump_bytes())
    finally:
        t.close()
    for a in (["-o", out + "2", even], ["-c", "0", "-o", out + "2", tab.fn], ["-c1024", "-o", out + "2", tab.fn]):
        r = subprocess.run([CLI, "hetmers"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out + "2"), a
