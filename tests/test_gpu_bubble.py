"""The simple bubbles on the device (the kernels of yak_amd/bubble/bubble.hip behind yakamd_bubble_open, yakamd_bubble_records_dev, yakamd_bubbles,
the CLI's `bubbles` and yak_amd.bubble) against the restatements of tests/bubble_util.py (held to each other, to hand-derived cases and to the
sequential model of the kernels by tests/test_bubble.py and tests/test_bubble_model.py), always on the dump of the very table that was walked: the
records field by field, the tallies, both texts byte for byte.  The hand cases at k = 5, a planted genome across the sub-tables of -p13, arms of
more than 64 and more than 256 bases, bubbles in several tiles of the scan, reads, cycles, a table without a node and every 7-mer; the size
queries, the records after the close of the walk and the links, the CLI and yak_amd.bubble, the names of `unitigs -G`, the pairs of `hetmers -p`,
the refusals, and a launch of every kernel of the library."""
import ctypes as C
import os
import random
import subprocess

import pytest

import bubble_util as B
import gfa_util as G
import graph_util as U
from test_bubble import HAND, PLANTED_SEEDS
from test_gpu_gfa import call_text, every_7_mer, genome
from test_gpu_graph import CLI, Tab, restated_file

pytestmark = pytest.mark.gpu
T = 600
KERNELS = {"k_bub_first", "k_bub_find<COUNT>", "k_bub_find<EMIT>", "k_bub_tile_sum", "k_bub_tile_scan", "k_bub_scan_apply", "k_bub_classify"}
NOTHING = dict(n_bubble=0, n_type=[0, 0, 0], n_tip=0, tip_nodes=0, max_arm_nodes=0, n_fork=0)


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the bubbles have no CPU fallback"
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


@pytest.fixture(scope="module")
def yb(yg):
    import yak_amd.bubble
    yak_amd.bubble.lib()
    return yak_amd.bubble


def snp_chains(k, runs, seed):
    """a random genome and a copy in which, for every m of runs, m bases k - 1 apart are changed: every k-mer around a chain holds at least one of
    them, so the chain is one bubble whose arms have k + (m - 1) (k - 1) nodes and differ in m places"""
    g = list(genome(200 + sum(3 * k + m * k for m in runs), seed).decode())
    h, p = list(g), 100
    rng = random.Random(seed)
    for m in runs:
        for i in range(m):
            h[p + i * (k - 1)] = rng.choice([c for c in "ACGT" if c != g[p + i * (k - 1)]])
        p += m * (k - 1) + 3 * k
    return U.image(["".join(g).encode(), "".join(h).encode()])


def many_snps(k, n, seed):
    """a random genome of n bases and a copy with every (2 k + 10)-th base changed"""
    g = genome(n, seed).decode()
    rng = random.Random(seed)
    h = list(g)
    for p in range(2 * k, n - 2 * k, 2 * k + 10):
        h[p] = rng.choice([c for c in "ACGT" if c != g[p]])
    return U.image([g.encode(), "".join(h).encode()])


# the tables of the hand cases: name of the table -> name in test_bubble.HAND
HAND_TABLES = dict(bubble="bubble", tip="tip", tiplong="tip_long_flank", closing="closing", threeway="three_way", armforks="arm_forks", deletion="deletion",
                   twosnps="two_snps", circle="circle", cyclesandlone="cycles_and_lone")


def hand_image(name):
    return lambda synth: U.image([s.encode() for s in HAND[name][1]])


SHAPES = {t + "_k5_p10": hand_image(h) for t, h in HAND_TABLES.items()}
SHAPES.update({
    "planted_k31_p13": lambda synth: U.image([s.encode() for s in B.planted(31, 1000, PLANTED_SEEDS[(31, False)])[0]]),
    "ring_k15_p10": lambda synth: U.image([s.encode() for s in B.planted(15, 1000, PLANTED_SEEDS[(15, True)], True)[0]]),
    "chains_k31_p10": lambda synth: snp_chains(31, (2, 9, 3), 26),
    "manysnps_k15_p10": lambda synth: many_snps(15, 30000, 15),
    "snps_k21_p10": lambda synth: many_snps(21, 12000, 21),
    "reads_k31_p10": lambda synth: synth(2000, 150),
    "cycles_k31_p10": lambda synth: U.image([genome(3000, 31), b"AC" * 20, genome(500, 5), b"ACG" * 14]),
    "every_k7_p10": lambda synth: every_7_mer(),
})


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("bubble")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](synth), int(k[1:]), int(pre[1:]))
            tab.bub_want = {}
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def want_of(tab, min_cnt):
    """(graph tallies, unitigs, links, records, stats) of the dump, computed once: the bubbles from the strings, and the same from the links"""
    if min_cnt not in tab.bub_want:
        recs, st, ug = tab.restated(min_cnt)
        links = G.links_by_strings(tab.k, ug)
        want, bs = B.by_strings(tab.k, ug)
        assert (want, bs) == B.by_links(tab.k, ug, links)
        B.check_invariants(tab.k, ug, want, bs)
        tab.bub_want[min_cnt] = (st, ug, links, want, bs)
    return tab.bub_want[min_cnt]


def rows(arr):
    return [(int(r["src"]), int(r["sink"]), int(r["arm"][0]), int(r["arm"][1]), int(r["n_node"][0]), int(r["n_node"][1]), int(r["kc"][0]), int(r["kc"][1]),
             int(r["hd"]), int(r["type"])) for r in arr]


def check(ya, yw, yg, yb, tab, min_cnt, tmp_path):
    st, ug, links, want, bs = want_of(tab, min_cnt)
    with yw.Walk(tab.t, min_cnt) as w, yg.Gfa(w, tab.k) as g, yb.Bubbles(w, g, tab.k) as b:
        got = b.stats()
        print("stats", got, "ms", yb.ms())
        arr = b.records()
    assert got == bs
    assert rows(arr) == B.as_rows(want)
    out = str(tmp_path / "o.txt")
    text = call_text(ya, yb.lib().yakamd_bubbles, tab.t.h, min_cnt, out)
    assert text == B.text(tab.k, min_cnt, ug, want)
    tx = call_text(ya, yb.lib().yakamd_bubbles, tab.t.h, min_cnt, out, stats=True)
    assert tx == B.stats_text(tab.k, min_cnt, st, ug, links, bs)
    below = call_text(ya, yg.lib().yakamd_unitigs_gfa, tab.t.h, min_cnt, out, stats=True)
    assert tx.startswith(below) and tx[len(below):] == B.stats_line(bs)
    return got, ug, want


@pytest.mark.parametrize("name", sorted(HAND_TABLES))
def test_hand_cases_at_k5(ya, yw, yg, yb, tabs, tmp_path, name):
    tab = tabs(name + "_k5_p10")
    got, ug, want = check(ya, yw, yg, yb, tab, 1, tmp_path)
    n_type = dict(bubble=[1, 0, 0], closing=[1, 0, 0], deletion=[0, 0, 1], twosnps=[0, 1, 0], circle=[1, 0, 0]).get(name, [0, 0, 0])
    assert got["n_type"] == n_type
    assert got["n_tip"] == dict(bubble=1, closing=1, tip=2, tiplong=1, threeway=1, armforks=2, deletion=1, twosnps=2).get(name, 0)
    if name in ("threeway", "armforks"):
        assert got["n_fork"] == 3
    if name == "circle":
        assert want[0][0] >> 1 == want[0][1] >> 1
    if name == "closing":
        assert check(ya, yw, yg, yb, tab, 2, tmp_path)[0] == NOTHING


def test_planted_genome_across_sub_tables(ya, yw, yg, yb, tabs, tmp_path):
    got, ug, want = check(ya, yw, yg, yb, tabs("planted_k31_p13"), 1, tmp_path)
    planted = B.planted(31, 1000, PLANTED_SEEDS[(31, False)])[1]
    assert B.found(want) == sorted(planted) and got["n_type"] == [sum(1 for p in planted if p[0] == c) for c in "SEI"]
    assert {a & 1 for r in want for a in r[2]} == {0, 1}, "arms of one orientation only"
    assert check(ya, yw, yg, yb, tabs("planted_k31_p13"), 2, tmp_path)[0] == NOTHING


def test_circular_genome(ya, yw, yg, yb, tabs, tmp_path):
    got, ug, want = check(ya, yw, yg, yb, tabs("ring_k15_p10"), 1, tmp_path)
    assert B.found(want) == sorted(B.planted(15, 1000, PLANTED_SEEDS[(15, True)], True)[1]) and got["n_tip"] == 0


def test_long_arms_take_several_strides(ya, yw, yg, yb, tabs, tmp_path):
    """chains of 2, 9 and 3 changed bases 30 apart at k = 31: arms of 61, 271 and 91 nodes, 91, 301 and 121 bases -- two, five and two strides of a wave"""
    got, ug, want = check(ya, yw, yg, yb, tabs("chains_k31_p10"), 1, tmp_path)
    assert sorted((r[3], r[5], r[6]) for r in want) == [((61, 61), 2, "E"), ((91, 91), 3, "E"), ((271, 271), 9, "E")]
    assert got["max_arm_nodes"] == 271 and got["n_type"] == [0, 3, 0]


def test_bubbles_in_several_tiles_of_the_scan(ya, yw, yg, yb, tabs, tmp_path):
    got, ug, want = check(ya, yw, yg, yb, tabs("manysnps_k15_p10"), 1, tmp_path)
    assert 2 * len(ug) > 3 * 1024 and got["n_bubble"] > 600 and got["n_type"][0] > 600
    assert len({r[0] // 1024 for r in want}) >= 3, "all sources in one tile of the scan"


@pytest.mark.parametrize("min_cnt", [1, 2])
def test_reads(ya, yw, yg, yb, tabs, tmp_path, min_cnt):
    got, ug, want = check(ya, yw, yg, yb, tabs("reads_k31_p10"), min_cnt, tmp_path)
    if min_cnt == 1:
        # an error every seven bases of the genome: the forks of one error cut the arms of the next, and hardly a bubble is simple
        assert got["n_fork"] > 500 and got["n_tip"] > 100 and got["n_bubble"] >= 1, got


def test_cycles_beside_open_unitigs(ya, yw, yg, yb, tabs, tmp_path):
    got, ug, want = check(ya, yw, yg, yb, tabs("cycles_k31_p10"), 1, tmp_path)
    assert sum(1 for u in ug if u[3]) == 2 and got == NOTHING


def test_a_table_without_a_node(ya, yw, yg, yb, tabs, tmp_path):
    tab = tabs("reads_k31_p10")
    got, ug, want = check(ya, yw, yg, yb, tab, 1023, tmp_path)
    assert ug == [] and got == NOTHING
    assert call_text(ya, yb.lib().yakamd_bubbles, tab.t.h, 1023, str(tmp_path / "e.txt")) == b"#bubbles\tk=31\tmin_cnt=1023\n"


def test_every_7_mer(ya, yw, yg, yb, tabs, tmp_path):
    """8192 unitigs of one node: 16 384 oriented ends in 16 tiles of the scan, every end a fork of four links, no bubble"""
    got, ug, want = check(ya, yw, yg, yb, tabs("every_k7_p10"), 1, tmp_path)
    assert got == dict(NOTHING, n_fork=16384)


def test_size_queries_write_nothing(ya, yw, yg, yb, tabs):
    L = ya.lib()
    tab = tabs("manysnps_k15_p10")
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 15) as g, yb.Bubbles(w, g, 15) as b:
        n = b.stats()["n_bubble"]
        get = b.L.yakamd_bubble_records_dev
        assert n > 0
        nb = n * 80 + 4096
        d = L.yakamd_dev_alloc(nb)
        assert d
        try:
            poison = bytes([0xA5]) * nb
            raw = C.create_string_buffer(nb)
            assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
            assert get(b.b, None, 0) == n == get(b.b, None, n) == get(b.b, d, n - 1) == get(b.b, d, 0)
            assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
            assert get(b.b, d, n + 7) == n
            assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
            assert raw.raw[n * 80:] == poison[n * 80:], "written past the last record"
            assert raw.raw[:n * 80] != poison[:n * 80]
            assert get(b.b, d + 8, n) == -1 and b"aligned" in b.L.yakamd_bubble_last_error()
        finally:
            L.yakamd_dev_free(d)


def test_the_records_outlive_the_walk_and_the_links(ya, yw, yg, yb, tabs):
    tab = tabs("chains_k31_p10")
    w = yw.Walk(tab.t, 1)
    g = yg.Gfa(w, 31)
    b = yb.Bubbles(w, g, 31)
    g.close()
    w.close()
    try:
        assert rows(b.records()) == B.as_rows(want_of(tab, 1)[3]) and b.stats() == want_of(tab, 1)[4]
    finally:
        b.close()


def test_cli_python_names_and_hetmers(ya, yw, yg, yb, tabs, tmp_path):
    """yakamd_bubbles, the CLI and yak_amd.bubble agree byte for byte; the u<j> are the S lines of `unitigs -G`; -s begins with `unitigs -G -s`; the
    middle k-mers of every S bubble are a pair of `hetmers -p`.  On reads, and on 12 000 bases with a changed base every 52 at k = 21"""
    n_s = sum(cli_python_names_and_hetmers(ya, yb, tabs(name), tmp_path) for name in ("reads_k31_p10", "snps_k21_p10"))
    assert n_s > 200


def cli_python_names_and_hetmers(ya, yb, tab, tmp_path):
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))      # the command restores the file: the listing order is that table's
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
        lib_text = {(c, s): call_text(ya, yb.lib().yakamd_bubbles, back.h, c, str(tmp_path / "l.txt"), stats=s) for c in (1, 2) for s in (False, True)}
    finally:
        back.close()
    run = lambda cmd, a: subprocess.run([CLI, cmd] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=T).stdout
    n_s = 0
    for min_cnt in (1, 2):
        k, recs, st, ug = restated_file(f, min_cnt)
        links = G.links_by_strings(k, ug)
        want, bs = B.by_strings(k, ug)
        c = ["-c%d" % min_cnt]
        text = run("bubbles", c + [tab.fn])
        assert text == B.text(k, min_cnt, ug, want) == yb.bubbles(tab.fn, min_cnt=min_cnt) == lib_text[(min_cnt, False)]
        tx = run("bubbles", c + ["-s", tab.fn])
        assert tx == B.stats_text(k, min_cnt, st, ug, links, bs) == yb.bubbles(tab.fn, min_cnt=min_cnt, stats_only=True) == lib_text[(min_cnt, True)]
        below = run("unitigs", c + ["-G", "-s", tab.fn])
        assert tx.startswith(below) and tx[len(below):] == B.stats_line(bs)
        seg = dict(G.parse_gfa(run("unitigs", c + ["-G", tab.fn]))[0])
        pairs = set()
        for ln in run("hetmers", c + ["-p", tab.fn]).decode().splitlines():
            fl = ln.split("\t")
            if fl[0] == "K":
                pairs.add(tuple(sorted((fl[1], fl[3]))))
        for ln in text.decode().splitlines()[1:]:
            fl = ln.split("\t")
            arms = [seg[e[:-1]] if e[-1] == "+" else U.rc_str(seg[e[:-1]]) for e in fl[3:5]]
            assert [len(a) - k + 1 for a in arms] == [int(fl[7]), int(fl[8])]
            assert [a[k - 1:len(a) - k + 1] or "*" for a in arms] == fl[12:14]
            src = seg[fl[2][:-1]] if fl[2][-1] == "+" else U.rc_str(seg[fl[2][:-1]])
            assert all(src[len(src) - (k - 1):] == a[:k - 1] for a in arms)
            if fl[6] == "S":
                n_s += 1
                assert tuple(sorted(U.canon(a[(k - 1) // 2:(k - 1) // 2 + k]) for a in arms)) in pairs
    out = str(tmp_path / "o.txt")
    assert run("bubbles", ["-c2", "-o", out, tab.fn]) == b"" and open(out, "rb").read() == text
    assert run("bubbles", ["-c1023", tab.fn]) == b"#bubbles\tk=%d\tmin_cnt=1023\n" % k and run("bubbles", ["-c1023", "-s", tab.fn]).endswith(b"\nG\t0\t0\t0\t0\t0\t0\nB\t0\t0\t0\t0\t0\t0\t0\t0\n")
    for a in (["-c", "0", "-o", out + "2", tab.fn], ["-c", "1024", "-o", out + "2", tab.fn], ["-o", out + "2", str(tmp_path / "nope.yak")]):
        r = subprocess.run([CLI, "bubbles"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out + "2"), a
    u = subprocess.run([CLI, "bubbles"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd bubbles")
    return n_s


def test_refusals(ya, yw, yg, yb, tabs, synth, tmp_path):
    BL = yb.lib()
    out = str(tmp_path / "o.txt")
    tab = tabs("reads_k31_p10")
    w2 = yw.Walk(tab.t, 2)
    g2 = yg.Gfa(w2, 31)                                            # the links of another walk: another number of unitigs
    w2.close()
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 31) as g:
        assert BL.yakamd_bubble_open(None, g.g, 31) is None and b"no walk" in BL.yakamd_bubble_last_error()
        assert BL.yakamd_bubble_open(w.w, None, 31) is None and b"no links" in BL.yakamd_bubble_last_error()
        for k, what in ((30, b"odd"), (2, b"odd"), (1, b"[3, 31]"), (33, b"[3, 31]"), (-5, b"[3, 31]"), (29, b"does not fit the walk"), (21, b"does not fit the walk")):
            assert BL.yakamd_bubble_open(w.w, g.g, k) is None and what in BL.yakamd_bubble_last_error(), (k, BL.yakamd_bubble_last_error())
        assert BL.yakamd_bubble_open(w.w, g2.g, 31) is None and b"the links are those of" in BL.yakamd_bubble_last_error()
        g2.close()
        st = yb.BubstatT()
        with yb.Bubbles(w, g, 31) as b:
            assert BL.yakamd_bubble_stats(b.b, None) == -1 and BL.yakamd_bubble_stats(None, C.byref(st)) == -1
    with yw.Walk(tab.t, 1023) as w, yg.Gfa(w, 5) as g, yb.Bubbles(w, g, 5) as b:      # a walk without unitigs fits every k, opens, and has no bubble
        assert b.stats() == NOTHING and len(b.records()) == 0
    o = ya.UgoptT()
    ya.lib().yakamd_ugopt_init(C.byref(o))
    for h, min_cnt, what in ((None, 1, b"not an engine table"), (tab.t.h, 0, b"min_cnt 0"), (tab.t.h, 1024, b"min_cnt 1024")):
        o.min_cnt = min_cnt
        assert BL.yakamd_bubbles(C.byref(o), h, out.encode()) == -1 and what in BL.yakamd_bubble_last_error()
        assert not os.path.exists(out), "a refused call created its output"
    t = ya.Table(30, 10, 4, 0)
    try:
        t.count_pass_host(1, synth(300, 150, 2500, s=5))
        o.min_cnt = 1
        assert BL.yakamd_bubbles(C.byref(o), t.h, out.encode()) == -1 and b"even" in BL.yakamd_bubble_last_error() and not os.path.exists(out)
    finally:
        t.close()


def test_every_kernel_is_launched_once_per_call(ya, yw, yg, yb, tabs):
    """the seven instantiations of the library's tally and no other launch: one open launches each of them once, and nothing of the libraries below"""
    assert set(yb.tally()) == KERNELS
    yb.lib().yakamd_bubble_tally_reset()
    assert not any(yb.tally().values())
    for i, name in enumerate(("bubble_k5_p10", "manysnps_k15_p10", "cyclesandlone_k5_p10")):
        tab = tabs(name)
        with yw.Walk(tab.t, 1) as w, yg.Gfa(w, tab.k) as g:
            before = (yw.tally(), yg.tally(), main_tally(ya))
            with yb.Bubbles(w, g, tab.k):
                pass
            assert (yw.tally(), yg.tally(), main_tally(ya)) == before      # the bubbles launch nothing of the layers below
        assert set(yb.tally().values()) == {i + 1}, yb.tally()
    with yw.Walk(tabs("reads_k31_p10").t, 1023) as w, yg.Gfa(w, 31) as g, yb.Bubbles(w, g, 31):     # no unitig: no launch
        pass
    assert set(yb.tally().values()) == {3}


def main_tally(ya):
    names = C.POINTER(C.c_char_p)()
    n = ya.lib().yakamd_tally_names(C.byref(names))
    out = (C.c_uint64 * n)()
    ya.lib().yakamd_tally_read(out, n)
    return {names[i].decode(): int(out[i]) for i in range(n)}
