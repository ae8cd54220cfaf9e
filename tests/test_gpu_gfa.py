"""The links between unitigs on the device (the kernels of yak_amd/gfa/gfa.hip behind yakamd_gfa_open, yakamd_gfa_links_dev, yakamd_unitigs_gfa, the
CLI's -G and yak_amd.gfa) against the restatements of tests/gfa_util.py (held to each other, to hand-derived cases and to the sequential model of
the kernels by tests/test_gfa.py and tests/test_gfa_model.py), always on the dump of the very table that was walked: the links element by element,
the tallies, both texts byte for byte; the S lines against the FASTA of `unitigs -g`; the identities against the graph's tallies as the walk keeps
them.  Tables of every degree, of one unitig without a link, of bubbles across sub-tables, of reads, of cycles, without a node, and of every 7-mer
-- 16 384 oriented ends, more than one tile of the scan, every end full -- also with the end table at its smallest capacity; of every 9-mer -- as
many tiles as the scan's workgroup has threads; the size queries, the refusals, and a launch of every kernel of the library."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import gfa_util as G
import graph_util as U
import walk_util as W
from test_gpu_graph import CLI, Tab, mixed_k5, restated_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the links have no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def yw(ya):
    import yak_amd.walk
    yak_amd.walk.lib()
    return yak_amd.walk


@pytest.fixture(scope="module")
def yg(yw):
    import yak_amd.gfa
    yak_amd.gfa.lib()
    return yak_amd.gfa


def genome(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


def snp_copies():
    """a 70 000-base genome and, around five of its positions, a copy of 200 bases with the middle base changed: five bubbles whose arms of 21
    nodes lie in other sub-tables than their flanks"""
    g = genome(70000, 70)
    recs = [g]
    for p in (5000, 20000, 35000, 50000, 65000):
        recs.append(g[p - 100:p] + {65: b"C", 67: b"G", 71: b"T", 84: b"A"}[g[p]] + g[p + 1:p + 100])
    return U.image(recs)


def every_7_mer():
    return U.image(["".join("ACGT"[i >> 2 * j & 3] for j in range(7)).encode() for i in range(1 << 14)])


def every_9_mer():
    """a de Bruijn sequence of order 9 over ACGT (the Lyndon words whose length divides 9, in order), its first 8 bases again behind it: 262 152
    bases in which every 9-mer stands once"""
    seq, a = [], [0] * 10

    def db(t, p):
        if t > 9:
            if 9 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    assert len(seq) == 4 ** 9
    return U.image([bytes(b"ACGT"[c] for c in seq + seq[:8])])


SHAPES = {
    "mixed_k5_p10": lambda synth: mixed_k5(),
    "genome3000_k31_p10": lambda synth: U.image([genome(3000, 31)]),
    "snps70000_k21_p13": lambda synth: snp_copies(),
    "reads_k31_p10": lambda synth: synth(2000, 150),
    "cycles_k31_p10": lambda synth: U.image([genome(3000, 31), b"AC" * 20, genome(500, 5), b"ACG" * 14]),
    "ac8_k5_p10": lambda synth: U.image([b"AC" * 8]),
    "every_k7_p10": lambda synth: every_7_mer(),
    "every_k9_p10": lambda synth: every_9_mer(),
}


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("gfa")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](synth), int(k[1:]), int(pre[1:]))
            tab.gfa_want = {}
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def want_of(tab, min_cnt):
    """(graph tallies, unitigs, links) of the dump, computed once: the links by strings, and the same from the records and the map"""
    if min_cnt not in tab.gfa_want:
        recs, st, ug = tab.restated(min_cnt)
        amap, desc, bases = W.restate(tab.k, recs, min_cnt, ug)
        links = G.links_by_strings(tab.k, ug)
        assert links == G.links_by_map(tab.k, recs, min_cnt, ug, amap)
        tab.gfa_want[min_cnt] = (st, ug, links)
    return tab.gfa_want[min_cnt]


def call_text(ya, lib_call, h, min_cnt, out, stats=False):
    o = ya.UgoptT()
    ya.lib().yakamd_ugopt_init(C.byref(o))
    o.min_cnt, o.stats_only, o.n_threads, o.batch_keys = min_cnt, int(stats), 0, 0
    if os.path.exists(out):
        os.remove(out)
    assert lib_call(C.byref(o), h, out.encode()) == 0
    return open(out, "rb").read()


def check(ya, yw, yg, tab, min_cnt, tmp_path, slots=None):
    st, ug, links = want_of(tab, min_cnt)
    n_cycle = sum(1 for u in ug if u[3])
    with yw.Walk(tab.t, min_cnt) as w:
        gst = w.gstat()
        with yg.Gfa(w, tab.k) as g:
            got = g.stats()
            print("stats", got)
            arr = g.links()
    assert gst == st
    assert len(arr) == len(links) == got["n_link"] == gst["n_arc"] - gst["n_linked_side"] + 2 * n_cycle
    want = np.array(links, np.uint64).reshape(-1, 2)
    assert np.array_equal(arr["from"], want[:, 0]) and np.array_equal(arr["to"], want[:, 1])
    deg = G.check_identities(gst, ug, [(int(f), int(t)) for f, t in zip(arr["from"], arr["to"])])
    assert got["end_deg"] == deg and sum(deg) == 2 * got["n_open"]
    assert (got["n_unitig"], got["n_open"], got["n_cycle"]) == (len(ug), len(ug) - n_cycle, n_cycle)
    n_key = G.n_keys(ug)
    if ug:                                                       # slots: what YAKAMD_GFA_SLOTS asks for, where the test has set it
        assert (got["table_slots"] >= 2 * n_key if slots is None else slots <= got["table_slots"] < 2 * slots) and n_key <= got["table_slots"]
        assert got["table_slots"] & (got["table_slots"] - 1) == 0 and got["max_probe"] <= got["table_slots"]
    out = str(tmp_path / "o.txt")
    text = call_text(ya, yg.lib().yakamd_unitigs_gfa, tab.t.h, min_cnt, out)
    assert text == G.gfa_text(tab.k, ug, links)
    fa = call_text(ya, yw.lib().yakamd_unitigs_dev, tab.t.h, min_cnt, out)
    assert [s for _, s in G.parse_gfa(text)[0]] == [ln.decode() for ln in fa.split(b"\n")[1::2]]
    tx = call_text(ya, yg.lib().yakamd_unitigs_gfa, tab.t.h, min_cnt, out, stats=True)
    assert tx == G.stats_text(tab.k, min_cnt, st, ug, links)
    assert tx.startswith(call_text(ya, yw.lib().yakamd_unitigs_dev, tab.t.h, min_cnt, out, stats=True)) and tx.count(b"\nG\t") == 1
    return got, ug, links


def test_every_degree_at_k5(ya, yw, yg, tabs, tmp_path):
    got, ug, links = check(ya, yw, yg, tabs("mixed_k5_p10"), 1, tmp_path)
    assert all(got["end_deg"]) and got["n_open"] > 100 and any((t ^ 1, f ^ 1) == (f, t) for f, t in links)
    check(ya, yw, yg, tabs("mixed_k5_p10"), 2, tmp_path)


def test_one_unitig_has_no_link(ya, yw, yg, tabs):
    tab = tabs("genome3000_k31_p10")
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 31) as g:
        got = g.stats()
        assert (got["n_unitig"], got["n_link"], got["end_deg"]) == (1, 0, [2, 0, 0, 0, 0]) and got["table_slots"] == 16
        assert len(g.links()) == 0
        d = ya.lib().yakamd_dev_alloc(4096)
        try:
            assert g.L.yakamd_gfa_links_dev(g.g, None, 0) == 0 == g.L.yakamd_gfa_links_dev(g.g, d, 100)      # zero-size getters
        finally:
            ya.lib().yakamd_dev_free(d)


def test_one_unitig_texts(ya, yw, yg, tabs, tmp_path):
    got, ug, links = check(ya, yw, yg, tabs("genome3000_k31_p10"), 1, tmp_path)
    assert len(ug) == 1 and links == []


def test_bubbles_across_sub_tables(ya, yw, yg, tabs, tmp_path):
    """five SNPs: 5 x 2 arms and 6 pieces of the genome between them, every fork an end of two links"""
    got, ug, links = check(ya, yw, yg, tabs("snps70000_k21_p13"), 1, tmp_path)
    assert got["n_open"] == 16 and got["n_link"] == 40 and got["end_deg"] == [2, 20, 10, 0, 0]
    assert sorted(u[1] for u in ug)[:10] == [21] * 10


@pytest.mark.parametrize("min_cnt", [1, 2])
def test_reads(ya, yw, yg, tabs, tmp_path, min_cnt):
    got, ug, links = check(ya, yw, yg, tabs("reads_k31_p10"), min_cnt, tmp_path)
    if min_cnt == 1:
        assert got["n_open"] > 2 * 1024 and got["n_link"] > 1000


def test_cycles(ya, yw, yg, tabs, tmp_path):
    got, ug, links = check(ya, yw, yg, tabs("cycles_k31_p10"), 1, tmp_path)
    assert (got["n_open"], got["n_cycle"]) == (2, 2) and links == [(4, 4), (5, 5), (6, 6), (7, 7)] and got["end_deg"] == [4, 0, 0, 0, 0]
    got, ug, links = check(ya, yw, yg, tabs("ac8_k5_p10"), 1, tmp_path)
    assert (got["n_open"], got["n_cycle"], got["table_slots"]) == (0, 1, 16) and links == [(0, 0), (1, 1)] and got["end_deg"] == [0] * 5


def test_a_table_without_a_node(ya, yw, yg, tabs, tmp_path):
    got, ug, links = check(ya, yw, yg, tabs("reads_k31_p10"), 1023, tmp_path)
    assert got == dict(n_unitig=0, n_open=0, n_cycle=0, n_link=0, end_deg=[0] * 5, table_slots=0, max_probe=0)
    assert call_text(ya, yg.lib().yakamd_unitigs_gfa, tabs("reads_k31_p10").t.h, 1023, str(tmp_path / "e.gfa")) == b"H\tVN:Z:1.0\n"


def test_every_7_mer(ya, yw, yg, tabs, tmp_path, monkeypatch):
    """8192 unitigs of one node, 16 384 oriented ends in 16 tiles of the scan, every end with four links; then the same with 8192 keys in 8192
    slots: no free slot is left, and the claims and the look-ups still end"""
    tab = tabs("every_k7_p10")
    got, ug, links = check(ya, yw, yg, tab, 1, tmp_path)
    assert got["n_open"] == 8192 and got["n_link"] == 65536 and got["end_deg"] == [0, 0, 0, 0, 16384] and got["table_slots"] == 16384
    monkeypatch.setenv("YAKAMD_GFA_SLOTS", "8192")
    full, _, _ = check(ya, yw, yg, tab, 1, tmp_path, slots=8192)
    assert full["table_slots"] == 8192 and full["max_probe"] > got["max_probe"]
    monkeypatch.setenv("YAKAMD_GFA_SLOTS", "8191")
    with yw.Walk(tab.t, 1) as w:
        assert yg.lib().yakamd_gfa_open(w.w, 7) is None and b"YAKAMD_GFA_SLOTS = 8191: the end table has 8192 keys" in yg.lib().yakamd_gfa_last_error()


def test_every_9_mer(ya, yw, yg, tabs):
    """131 072 unitigs of one node: 262 144 oriented ends are exactly 256 tiles of 1024, so that each of the 256 threads of k_gfa_tile_scan owns one
    tile and the clamp of its slice sits on the slice's edge.  Every end has four links, so end e must own the entries 4e .. 4e + 3 of the list: an
    offset that is wrong at any tile's edge moves them.  (The restatement in Python is not run at this size.)"""
    tab = tabs("every_k9_p10")
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 9) as g:
        got = g.stats()
        arr = g.links()
    print("stats", got)
    assert got["n_open"] == 131072
    assert got["n_link"] == 1048576
    assert got["end_deg"] == [0, 0, 0, 0, 262144]
    assert len(arr) == 1048576 and np.array_equal(arr["from"], np.repeat(np.arange(262144, dtype=np.uint64), 4))


def test_smallest_capacity_with_chains(ya, yw, yg, tabs, tmp_path, monkeypatch):
    """the k5 table at a capacity equal to its number of keys, rounded up to the next power of two"""
    tab = tabs("mixed_k5_p10")
    n_key = G.n_keys(want_of(tab, 1)[1])
    monkeypatch.setenv("YAKAMD_GFA_SLOTS", str(n_key))
    got, _, _ = check(ya, yw, yg, tab, 1, tmp_path, slots=n_key)
    assert n_key <= got["table_slots"] < 2 * n_key


def test_size_queries_write_nothing(ya, yw, yg, tabs):
    L = ya.lib()
    tab = tabs("reads_k31_p10")
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 31) as g:
        n = g.stats()["n_link"]
        get = g.L.yakamd_gfa_links_dev
        assert n > 0
        nb = n * 16 + 4096
        d = L.yakamd_dev_alloc(nb)
        assert d
        try:
            poison = bytes([0xA5]) * nb
            raw = C.create_string_buffer(nb)
            assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
            assert get(g.g, None, 0) == n == get(g.g, None, n) == get(g.g, d, n - 1) == get(g.g, d, 0)
            assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
            assert get(g.g, d, n + 7) == n
            assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
            assert raw.raw[n * 16:] == poison[n * 16:], "written past the last link"
            assert raw.raw[:n * 16] != poison[:n * 16]
            assert get(g.g, d + 8, n) == -1 and b"aligned" in g.L.yakamd_gfa_last_error()
        finally:
            L.yakamd_dev_free(d)


def test_the_links_outlive_the_walk(ya, yw, yg, tabs):
    tab = tabs("mixed_k5_p10")
    w = yw.Walk(tab.t, 1)
    g = yg.Gfa(w, 5)
    w.close()
    try:
        assert [(int(f), int(t)) for f, t in g.links()] == want_of(tab, 1)[2]
    finally:
        g.close()


def test_cli_and_python(ya, yw, yg, tabs, tmp_path):
    tab = tabs("reads_k31_p10")
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))      # the command restores the file: the listing order is that table's
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
    finally:
        back.close()
    run = lambda a: subprocess.run([CLI, "unitigs"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    for min_cnt in (1, 2):
        k, recs, st, ug = restated_file(f, min_cnt)
        links = G.links_by_strings(k, ug)
        c = ["-c%d" % min_cnt]
        assert run(c + ["-G", tab.fn]) == G.gfa_text(k, ug, links) == yg.gfa(tab.fn, min_cnt=min_cnt)
        assert run(c + ["-sG", tab.fn]) == G.stats_text(k, min_cnt, st, ug, links) == yg.gfa(tab.fn, min_cnt=min_cnt, stats_only=True)
    assert run(c + ["-g", "-s", tab.fn]) == U.stats_text(k, 2, st, ug) and run(c + ["-g", tab.fn]) == U.fasta_text(ug)      # nothing changes without -G
    out = str(tmp_path / "o.gfa")
    assert run(["-g", "-G", "-c2", "-o", out, tab.fn]) == b"" and open(out, "rb").read() == G.gfa_text(k, ug, links)
    assert run(["-G", "-c1023", tab.fn]) == b"H\tVN:Z:1.0\n" and run(["-G", "-c1023", "-s", tab.fn]).endswith(b"\nU\t0\t0\t0\t0\t0\nG\t0\t0\t0\t0\t0\t0\n")
    for a in (["-G", "-c", "0", "-o", out + "2", tab.fn],):
        r = subprocess.run([CLI, "unitigs"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out + "2"), a
    r = subprocess.run([CLI, "unitigs", "-G", "-o", out + "2", tab.fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, YAKAMD_GFA_SLOTS="1"))
    assert r.returncode == 3 and b"YAKAMD_GFA_SLOTS = 1" in r.stderr and not os.path.exists(out + "2")


def test_refusals(ya, yw, yg, tabs, synth, tmp_path):
    GL = yg.lib()
    out = str(tmp_path / "o.txt")
    tab = tabs("reads_k31_p10")
    assert GL.yakamd_gfa_open(None, 31) is None and b"no walk" in GL.yakamd_gfa_last_error()
    with yw.Walk(tab.t, 1) as w:
        for k, what in ((30, b"odd"), (2, b"odd"), (1, b"[3, 31]"), (33, b"[3, 31]"), (-5, b"[3, 31]"), (29, b"does not fit the walk"), (21, b"does not fit the walk")):
            assert GL.yakamd_gfa_open(w.w, k) is None and what in GL.yakamd_gfa_last_error(), (k, GL.yakamd_gfa_last_error())
        st = yg.GfastatT()
        with yg.Gfa(w, 31) as g:
            assert GL.yakamd_gfa_stats(g.g, None) == -1 and GL.yakamd_gfa_stats(None, C.byref(st)) == -1
    with yw.Walk(tab.t, 1023) as w, yg.Gfa(w, 5) as g:                 # a walk without unitigs fits every k, opens, and has no link
        assert g.stats()["n_link"] == 0 and len(g.links()) == 0
    o = ya.UgoptT()
    ya.lib().yakamd_ugopt_init(C.byref(o))
    for h, min_cnt, what in ((None, 1, b"not an engine table"), (tab.t.h, 0, b"min_cnt 0"), (tab.t.h, 1024, b"min_cnt 1024")):
        o.min_cnt = min_cnt
        assert GL.yakamd_unitigs_gfa(C.byref(o), h, out.encode()) == -1 and what in GL.yakamd_gfa_last_error()
        assert not os.path.exists(out), "a refused call created its output"
    t = ya.Table(30, 10, 4, 0)
    try:
        t.count_pass_host(1, synth(300, 150, 2500, s=5))
        o.min_cnt = 1
        assert GL.yakamd_unitigs_gfa(C.byref(o), t.h, out.encode()) == -1 and b"even" in GL.yakamd_gfa_last_error() and not os.path.exists(out)
    finally:
        t.close()


def test_every_kernel_is_launched(ya, yw, yg, tabs):
    """the six instantiations of the library's tally and no other launch: one call launches each of them once"""
    names = set(yg.tally())
    assert names == {"k_gfa_ends", "k_gfa_links<COUNT>", "k_gfa_links<EMIT>", "k_gfa_tile_sum", "k_gfa_tile_scan", "k_gfa_scan_apply"}
    yg.lib().yakamd_gfa_tally_reset()
    assert not any(yg.tally().values())
    before_walk, before_main = None, None
    for i, name in enumerate(("mixed_k5_p10", "every_k7_p10", "ac8_k5_p10")):
        with yw.Walk(tabs(name).t, 1) as w:
            before_walk = yw.tally()
            with yg.Gfa(w, tabs(name).k):
                pass
            assert yw.tally() == before_walk                      # the links launch nothing of the walk's
        assert set(yg.tally().values()) == {i + 1}, yg.tally()
    with yw.Walk(tabs("reads_k31_p10").t, 1023) as w, yg.Gfa(w, 31):     # no unitig: no launch
        pass
    assert set(yg.tally().values()) == {3}
