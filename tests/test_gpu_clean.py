"""The cleaning of the unitig graph on the device (the kernels of yak_amd/clean/clean.hip behind yakamd_clean_open, yakamd_clean_records_dev,
yakamd_clean_image_dev, yakamd_clean_round, yakamd_clean, the CLI's `clean` and yak_amd.clean) against the restatements of tests/clean_util.py (held
to each other, to hand-derived cases and to the sequential model of the kernels by tests/test_clean.py and tests/test_clean_model.py), always on the
dump of the very table that was walked: the records field by field, the image byte for byte, the tallies equal, round after round.  The hand cases at
k = 5, the planted reads across the sub-tables of -p13, tips around the image kernel's wave stride, popped arms of 271 nodes, more than 1024
removals, reads, every 7-mer and a table without a node; the size queries, the results after the close of the layers below, the command -- its
report byte for byte and its .yak byte for byte against the oracle's shrink / count / subtract sequence --, the CLI and yak_amd.clean, the refusals,
and a launch of every kernel of the library."""
import ctypes as C
import os
import random
import subprocess

import pytest

import bubble_util as B
import clean_util as K
import gfa_util as G
import graph_util as U
from test_clean import CASES, KERNELS, PLANTED
from test_gpu_bubble import many_snps, snp_chains
from test_gpu_gfa import every_7_mer, genome
from test_gpu_graph import CLI, restated_file

pytestmark = pytest.mark.gpu
TMO = 600
NOTHING = dict(n_tip=0, tip_nodes=0, n_tip_kept=0, n_pop=0, pop_nodes=0, n_pop_kept=0, n_rec=0, img_bytes=0)


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the cleaning has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def yc(ya):
    import yak_amd.clean
    yak_amd.clean.lib()
    return yak_amd.clean


def unequal(img, copies=3):
    """the image of two records with the first one `copies` times: its arms win every bubble"""
    g, h = img.split(b"\n")[:2]
    return U.image([g] * copies + [h])


def tips_of(k, sizes, seed):
    """three copies of a random genome and, every 150 bases, a record that follows it for k - 1 bases and then leaves it for m random ones: a tip of m
    nodes for every m of sizes"""
    rng = random.Random(seed + 1000)                             # not the genome's stream again
    g = genome(200 + 150 * len(sizes), seed).decode()
    recs = [g] * 3
    for i, m in enumerate(sizes):
        p = 100 + 150 * i
        tail = rng.choice([b for b in "ACGT" if b != g[p]]) + "".join(rng.choice("ACGT") for _ in range(m - 1))
        recs.append(g[p - (k - 1):p] + tail)
    return U.image([r.encode() for r in recs])


SHAPES = {name + "_k5_p10": (lambda n: lambda synth: U.image([s.encode() for s in CASES[n][0]]))(name) for name in CASES if name != "every_5_mer"}
SHAPES.update({
    "planted_k31_p13": lambda synth: U.image([r.encode() for r in K.planted_reads(31, dict(PLANTED)[31])[1]]),
    "planted_k15_p10": lambda synth: U.image([r.encode() for r in K.planted_reads(15, dict(PLANTED)[15])[1]]),
    "tips_k31_p10": lambda synth: tips_of(31, (1, 33, 34, 35, 63, 64, 65), 29),
    "chains_k31_p10": lambda synth: unequal(snp_chains(31, (2, 9, 3), 26)),
    "manysnps_k15_p10": lambda synth: unequal(many_snps(15, 50000, 15), 2),
    "reads_k31_p10": lambda synth: synth(2000, 150),
    "every_k7_p10": lambda synth: every_7_mer(),
})


def fresh(ya, synth, name):
    """a newly counted table: the rounds change it"""
    _, k, pre = name.rsplit("_", 2)
    t = ya.Table(int(k[1:]), int(pre[1:]), 4, 0)
    t.count_pass_host(1, SHAPES[name](synth))
    return t, int(k[1:])


def members_of(t, tmp_path, name="t.yak"):
    fn = str(tmp_path / name)
    open(fn, "wb").write(t.dump_bytes())
    kk, x, c = U.members(fn)
    return x, c


def rows(arr):
    return [tuple(int(r[f]) for f in ("unitig", "why", "n_node", "kc", "other", "off")) for r in arr]


def open_and_check(ya, yc, t, k, min_cnt, T, P, tmp_path, both=True):
    """the decisions of one round on the table as it is, against the restatement of its dump; returns the restated round"""
    import yak_amd.bubble as yb
    import yak_amd.gfa as yg
    import yak_amd.walk as yw
    x, c = members_of(t, tmp_path)
    d = K.one_round(k, x, c, min_cnt, T, P, both)
    with yw.Walk(t, min_cnt) as w, yg.Gfa(w, k) as g, yb.Bubbles(w, g, k) as b, yc.Clean(w, g, b, k, T, P) as cl:
        st, arr, img = cl.stats(), cl.records(), cl.image()
        print("stats", st, "ms", yc.ms())
    assert st == dict(d["stats"], n_rec=len(d["recs"]), img_bytes=len(d["image"]))
    assert rows(arr) == K.as_rows(k, d["recs"])
    assert img == d["image"]
    return d


def rounds_and_check(ya, yc, t, k, min_cnt, T, P, tmp_path, both=True, max_rounds=8):
    """yakamd_clean_round until nothing goes, every round against the restatement of the dump before it and the dump after it; the restated rounds"""
    done = []
    for r in range(max_rounds):
        d = open_and_check(ya, yc, t, k, min_cnt, T, P, tmp_path, both)
        x, c = members_of(t, tmp_path)
        before = t.dump_bytes()
        got = yc.clean_round(t, min_cnt, T, P)
        assert got == d["round"]
        after = K.table_set(k, *members_of(t, tmp_path))
        assert after == {(s, n) for s, n in K.table_set(k, x, c) if K.kmer_int(s) not in d["gone"]}
        assert t.tot == len(after)
        done.append(d)
        if not d["gone"]:
            assert t.dump_bytes() == before, "a round that removes nothing touched the table"
            break
    return done


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "every_5_mer"))
def test_hand_cases_at_k5(ya, yc, synth, tmp_path, name):
    t, k = fresh(ya, synth, name + "_k5_p10")
    try:
        done = rounds_and_check(ya, yc, t, 5, 1, 5, CASES[name][1], tmp_path)
        want = dict(tip=[2, 0], tip_long_flank=[2, 0], siblings=[2, 0], siblings_equal=[2, 0], three_way_tip=[2, 0], tip_minus=[2, 0], both_sides=[2, 0], short_alone=[0],
                    bubble31=[5, 0], bubble_equal=[5, 0], pct30=[0], pct40=[5, 0], deletion=[5, 0], circle=[5, 0], three_way=[0], arm_forks=[2, 5, 0], cycles_and_lone=[0])
        removed = [d["round"]["removed"] for d in done]
        # the deletion's arms have equal coverage, 4 nodes against 5: which of them is a2 depends on the side that reports, and so on the numbering
        assert removed == want[name] or (name == "deletion" and removed == [4, 0])
    finally:
        t.close()


@pytest.mark.parametrize("name", ["planted_k31_p13", "planted_k15_p10"])
def test_planted_reads_leave_the_genome(ya, yc, synth, tmp_path, name):
    t, k = fresh(ya, synth, name)
    try:
        x, c = members_of(t, tmp_path)
        done = rounds_and_check(ya, yc, t, k, 1, k, 100, tmp_path)
        assert [(d["round"]["n_tip"], d["round"]["n_pop"]) for d in done] == [(8, 12), (0, 0)] and len(done[1]["ug"]) == 1
        g = K.planted_reads(k, dict(PLANTED)[k])[0]
        genome_set = {U.canon(g[i:i + k]) for i in range(len(g) - k + 1)}
        assert K.table_set(k, *members_of(t, tmp_path)) == {(s, n) for s, n in K.table_set(k, x, c) if s in genome_set}
    finally:
        t.close()


def test_tips_around_the_wave_stride(ya, yc, synth, tmp_path):
    """tips of 1, 33, 34, 35, 63, 64 and 65 nodes at k = 31 with tip_nodes 100: 31, 63, 64, 65, 93, 94 and 95 bases, below, at and above one and two
    strides of the image kernel's wave"""
    t, k = fresh(ya, synth, "tips_k31_p10")
    try:
        done = rounds_and_check(ya, yc, t, 31, 1, 100, 100, tmp_path)
        assert sorted(r[2] for r in done[0]["recs"]) == [1, 33, 34, 35, 63, 64, 65] and all(r[1] == K.TIP for r in done[0]["recs"])
        assert [d["round"]["removed"] for d in done] == [295, 0] and len(done[1]["ug"]) == 1
        t2, _ = fresh(ya, synth, "tips_k31_p10")
        try:                                                     # the default tip_nodes = k clips the tip of one node alone
            assert [r[2] for r in open_and_check(ya, yc, t2, 31, 1, 31, 100, tmp_path)["recs"]] == [1]
        finally:
            t2.close()
    finally:
        t.close()


def test_long_popped_arms(ya, yc, synth, tmp_path):
    """the chains of 2, 9 and 3 changed bases at k = 31, the first record three times: the arms of 61, 271 and 91 nodes seen once are popped -- 301
    bases, more than one pass of a workgroup of 256 threads and five strides of a wave"""
    t, k = fresh(ya, synth, "chains_k31_p10")
    try:
        done = rounds_and_check(ya, yc, t, 31, 1, 31, 100, tmp_path)
        assert sorted((r[1], r[2], r[3]) for r in done[0]["recs"]) == [(K.POP, 61, 61), (K.POP, 91, 91), (K.POP, 271, 271)]
        assert [d["round"]["removed"] for d in done] == [423, 0]
        t2, _ = fresh(ya, synth, "chains_k31_p10")
        try:                                                     # 1 : 3 is above 30 per cent
            d = open_and_check(ya, yc, t2, 31, 1, 31, 30, tmp_path)
            assert d["recs"] == [] and d["stats"]["n_pop_kept"] == 3
        finally:
            t2.close()
    finally:
        t.close()


def test_removals_in_several_tiles_of_the_scan(ya, yc, synth, tmp_path):
    t, k = fresh(ya, synth, "manysnps_k15_p10")
    try:
        d = open_and_check(ya, yc, t, 15, 1, 15, 100, tmp_path)
        assert len(d["recs"]) > 1024 and len({r[0] // 1024 for r in d["recs"]}) >= 3 and d["round"]["n_pop"] > 1024, d["round"]
        done = rounds_and_check(ya, yc, t, 15, 1, 15, 100, tmp_path, both=False, max_rounds=2)
        assert done[0]["round"]["removed"] > 15 * 1024
    finally:
        t.close()


@pytest.mark.parametrize("min_cnt", [1, 2])
def test_reads(ya, yc, synth, tmp_path, min_cnt):
    t, k = fresh(ya, synth, "reads_k31_p10")
    try:
        if min_cnt > 1:
            t.shrink(min_cnt, 1023)
        done = rounds_and_check(ya, yc, t, 31, min_cnt, 31, 100, tmp_path, both=False, max_rounds=3)
        if min_cnt == 1:
            assert done[0]["round"]["n_tip"] > 100 and done[0]["stats"]["n_tip_kept"] > 0, done[0]["round"]
    finally:
        t.close()


def test_every_7_mer_and_a_table_without_a_node(ya, yc, synth, tmp_path):
    """8192 unitigs of one node with four links an end: nothing goes, no D is built and the table is not touched; at min_cnt 1023 there is no unitig"""
    t, k = fresh(ya, synth, "every_k7_p10")
    try:
        main_before = main_tally(ya)
        done = rounds_and_check(ya, yc, t, 7, 1, 7, 100, tmp_path, both=False)
        assert len(done) == 1 and done[0]["round"] == dict(n_key=8192, n_unitig=8192, n_link=65536, n_bubble=0, n_tip=0, tip_nodes=0, n_pop=0, pop_nodes=0, removed=0)
        xpart = lambda tl: {n: v for n, v in tl.items() if n.startswith("k_xpart")}
        assert xpart(main_tally(ya)) == xpart(main_before), "an extraction kernel ran: D was built"
        d = open_and_check(ya, yc, t, 7, 1023, 7, 100, tmp_path)
        assert d["ug"] == [] and d["recs"] == []
        assert yc.clean_round(t, 1023, 7, 100) == dict(n_key=8192, n_unitig=0, n_link=0, n_bubble=0, n_tip=0, tip_nodes=0, n_pop=0, pop_nodes=0, removed=0)
    finally:
        t.close()


def test_size_queries_write_nothing(ya, yc, synth):
    import yak_amd.bubble as yb
    import yak_amd.gfa as yg
    import yak_amd.walk as yw
    L = ya.lib()
    t, k = fresh(ya, synth, "chains_k31_p10")
    try:
        with yw.Walk(t, 1) as w, yg.Gfa(w, 31) as g, yb.Bubbles(w, g, 31) as b, yc.Clean(w, g, b, 31) as cl:
            st = cl.stats()
            for get, n, size in ((cl.L.yakamd_clean_records_dev, st["n_rec"], 48), (cl.L.yakamd_clean_image_dev, st["img_bytes"], 1)):
                assert n > 0
                nb = n * size + 4096
                d = L.yakamd_dev_alloc(nb)
                assert d
                try:
                    poison = bytes([0xA5]) * nb
                    raw = C.create_string_buffer(nb)
                    assert L.yakamd_memcpy_h2d(d, poison, nb) == 0
                    assert get(cl.c, None, 0) == n == get(cl.c, None, n) == get(cl.c, d, n - 1) == get(cl.c, d, 0)
                    assert L.yakamd_memcpy_d2h(raw, d, nb) == 0 and raw.raw == poison, "a size query wrote"
                    assert get(cl.c, d, n + 7) == n
                    assert L.yakamd_memcpy_d2h(raw, d, nb) == 0
                    assert raw.raw[n * size:] == poison[n * size:], "written past the last entry"
                    assert raw.raw[:n * size] != poison[:n * size]
                    assert get(cl.c, d + 8, n) == -1 and b"aligned" in cl.L.yakamd_clean_last_error()
                finally:
                    L.yakamd_dev_free(d)
    finally:
        t.close()


def test_the_results_outlive_the_layers_below(ya, yc, synth, tmp_path):
    import yak_amd.bubble as yb
    import yak_amd.gfa as yg
    import yak_amd.walk as yw
    t, k = fresh(ya, synth, "planted_k15_p10")
    try:
        x, c = members_of(t, tmp_path)
        d = K.one_round(15, x, c, 1, 15, 100)
        w = yw.Walk(t, 1)
        g = yg.Gfa(w, 15)
        b = yb.Bubbles(w, g, 15)
        cl = yc.Clean(w, g, b, 15)
        b.close(); g.close(); w.close()
        try:
            assert rows(cl.records()) == K.as_rows(15, d["recs"]) and cl.image() == d["image"] and cl.stats()["n_rec"] == len(d["recs"]) == 20
        finally:
            cl.close()
    finally:
        t.close()


# ---- the command ----
def oracle_clean(oracle, in_fn, tmp_path, min_cnt, T, P, max_rounds=8):
    """the oracle's sequence on a .yak file: restore, shrink, and per round the drop image of the restated decisions counted into D and subtracted.
    (the restated rounds, n_in, n_shrunk, n_out, the bytes of the dump)"""
    L = oracle.lib()
    t = L.yko_ch_restore(in_fn.encode())
    assert t
    k, pre, n_in = t.contents.k, t.contents.pre, len(U.members(in_fn)[1])      # a restored table does not say in `tot` how many keys it holds
    n_shrunk = n_out = n_in
    if min_cnt > 1:
        L.yko_ch_shrink(t, min_cnt, 1023)
        n_shrunk = n_out = t.contents.tot
    o = oracle.copt(k=k, pre=pre)
    fn = str(tmp_path / "oracle_round.yak")
    done = []
    for r in range(max_rounds):
        assert L.yko_ch_dump(t, fn.encode()) == 0
        kk, x, c = U.members(fn)
        d = K.one_round(k, x, c, min_cnt, T, P, both=len(x) < 20000)
        done.append(d)
        if not d["gone"]:
            break
        drop = L.yko_count_mem(d["image"], len(d["image"]), C.byref(o), None)
        assert drop.contents.tot == len(d["gone"])
        L.yko_ch_subtract(t, drop)
        L.yko_ch_destroy(drop)
        n_out = t.contents.tot
    out = oracle.dump_bytes(t)
    L.yko_ch_destroy(t)
    return done, n_in, n_shrunk, n_out, out


@pytest.mark.parametrize("name,min_cnt,T,P", [("arm_forks_k5_p10", 1, None, 100), ("planted_k31_p13", 1, None, 100), ("reads_k31_p10", 1, None, 100),
                                              ("reads_k31_p10", 2, 40, 60), ("chains_k31_p10", 1, 0, 30), ("manysnps_k15_p10", 1, None, 100)])
def test_command_cli_and_python(ya, yc, oracle, synth, tmp_path, name, min_cnt, T, P):
    """yakamd_clean, the CLI and yak_amd.clean: the report byte for byte against the restatement, the .yak byte for byte against the oracle's
    sequence; `bubbles -s` and `unitigs -G -s` of the output against the restatement of the surviving set"""
    t, k = fresh(ya, synth, name)
    in_fn = str(tmp_path / "in.yak")
    open(in_fn, "wb").write(t.dump_bytes())
    t.close()
    Tn = k if T is None else T
    done, n_in, n_shrunk, n_out, want_yak = oracle_clean(oracle, in_fn, tmp_path, min_cnt, Tn, P)
    run = lambda cmd, a: subprocess.run([CLI, cmd] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=TMO).stdout
    opts = ["-c%d" % min_cnt, "-b%d" % P] + ([] if T is None else ["-t%d" % T])
    for listed in (False, True):
        want = K.report(k, min_cnt, Tn, P, done, n_in, n_shrunk, n_out, listed)
        out, rep = str(tmp_path / "cli.yak"), str(tmp_path / "cli.txt")
        assert run("clean", opts + (["-l"] if listed else []) + [in_fn, out]) == want and open(out, "rb").read() == want_yak
        assert run("clean", opts + (["-l"] if listed else []) + ["-o", rep, in_fn, out]) == b"" and open(rep, "rb").read() == want
        py = str(tmp_path / "py.yak")
        assert yc.clean(in_fn, py, min_cnt, T, P, list_removed=listed) == want and open(py, "rb").read() == want_yak
    one = K.report(k, min_cnt, Tn, P, done[:1], n_in, n_shrunk, n_shrunk - done[0]["round"]["removed"])
    assert run("clean", opts + ["-r1", in_fn, str(tmp_path / "one.yak")]) == one
    # the cleaned table under the commands that read a table
    kk, recs, st, ug = restated_file(out, min_cnt)
    links = G.links_by_strings(kk, ug)
    bub, bs = B.by_links(kk, ug, links)
    assert run("bubbles", ["-c%d" % min_cnt, "-s", out]) == B.stats_text(kk, min_cnt, st, ug, links, bs)
    assert run("unitigs", ["-c%d" % min_cnt, "-G", "-s", out]) == G.stats_text(kk, min_cnt, st, ug, links)
    if not done[-1]["gone"]:
        assert (len(ug), len(links), len(bub)) == tuple(done[-1]["round"][f] for f in ("n_unitig", "n_link", "n_bubble"))
        again = run("clean", opts + [out, str(tmp_path / "again.yak")]).decode().splitlines()
        assert again[1].split("\t")[-1] == "0" and again[-1] == "C\t1\t%d\t%d\t%d" % (n_out, n_out, n_out)
        assert K.table_set(kk, *U.members(str(tmp_path / "again.yak"))[1:]) ==K.table_set(kk, *U.members(out)[1:])      # the same k-mers; a restore lays them out anew


def test_refusals_leave_no_file(ya, yc, synth, tmp_path):
    import yak_amd.bubble as yb
    import yak_amd.gfa as yg
    import yak_amd.walk as yw
    CL = yc.lib()
    err = CL.yakamd_clean_last_error
    t, k = fresh(ya, synth, "reads_k31_p10")
    out, rep = str(tmp_path / "o.yak"), str(tmp_path / "r.txt")
    try:
        w2 = yw.Walk(t, 2)
        g2 = yg.Gfa(w2, 31)
        b2 = yb.Bubbles(w2, g2, 31)                                 # the links and bubbles of another walk
        w2.close()
        with yw.Walk(t, 1) as w, yg.Gfa(w, 31) as g, yb.Bubbles(w, g, 31) as b:
            assert CL.yakamd_clean_open(None, g.g, b.b, 31, 31, 100) is None and b"no walk" in err()
            assert CL.yakamd_clean_open(w.w, None, b.b, 31, 31, 100) is None and b"no links" in err()
            assert CL.yakamd_clean_open(w.w, g.g, None, 31, 31, 100) is None and b"no bubbles" in err()
            for kk, what in ((30, b"odd"), (1, b"[3, 31]"), (33, b"[3, 31]"), (29, b"does not fit the walk")):
                assert CL.yakamd_clean_open(w.w, g.g, b.b, kk, 31, 100) is None and what in err(), (kk, err())
            for T, P, what in ((-1, 100, b"tip_nodes"), ((1 << 20) + 1, 100, b"tip_nodes"), (31, -1, b"pop_pct"), (31, 101, b"pop_pct")):
                assert CL.yakamd_clean_open(w.w, g.g, b.b, 31, T, P) is None and what in err(), (T, P, err())
            assert CL.yakamd_clean_open(w.w, g2.g, b.b, 31, 31, 100) is None and b"the links are those of" in err()
            assert CL.yakamd_clean_open(w.w, g.g, b2.b, 31, 31, 100) is None and b"bubbles" in err()
            with yc.Clean(w, g, b, 31, 1 << 20, 0) as cl:              # the ends of both ranges open
                assert CL.yakamd_clean_stats(cl.c, None) == -1 and cl.stats()["n_pop"] == 0
        b2.close(); g2.close()
        before = t.dump_bytes()
        for o, what in ((yc.options(min_cnt=0), b"min_cnt 0"), (yc.options(min_cnt=1024), b"min_cnt 1024"), (yc.options(tip_nodes=-2), b"tip_nodes"),
                        (yc.options(pop_pct=101), b"pop_pct"), (yc.options(max_rounds=0), b"max_rounds"), (yc.options(max_rounds=65), b"max_rounds")):
            assert CL.yakamd_clean(C.byref(o), t.h, out.encode(), rep.encode()) == -1 and what in err(), err()
            assert CL.yakamd_clean_round(t.h, C.byref(o), None) == -1 and what in err()
            assert not os.path.exists(out) and not os.path.exists(rep), "a refused call created an output"
        assert CL.yakamd_clean(C.byref(yc.options()), t.h, None, rep.encode()) == -1 and b"no name" in err() and not os.path.exists(rep)
        assert t.dump_bytes() == before
    finally:
        t.close()
    te = ya.Table(30, 10, 4, 0)
    try:
        te.count_pass_host(1, synth(300, 150, 2500, s=5))
        o = yc.options()
        assert CL.yakamd_clean(C.byref(o), te.h, out.encode(), rep.encode()) == -1 and b"even" in err()
        assert CL.yakamd_clean_round(te.h, C.byref(o), None) == -1 and b"even" in err()
        assert not os.path.exists(out) and not os.path.exists(rep)
    finally:
        te.close()
    for a in (["-c", "0"], ["-t", "-2"], ["-b", "101"], ["-r", "65"]):
        r = subprocess.run([CLI, "clean"] + a + ["-o", rep, str(tmp_path / "nope.yak"), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TMO)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out) and not os.path.exists(rep), a
    u = subprocess.run([CLI, "clean"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd clean")


def test_every_kernel_is_launched_once_per_open(ya, yc, synth):
    """the nine instantiations of the library's tally and no other launch: one open launches each of them once and nothing of the libraries below; a
    walk without unitigs launches none"""
    import yak_amd.bubble as yb
    import yak_amd.gfa as yg
    import yak_amd.walk as yw
    assert set(yc.tally()) == set(KERNELS)
    yc.lib().yakamd_clean_tally_reset()
    assert not any(yc.tally().values())
    for i, name in enumerate(("bubble31_k5_p10", "manysnps_k15_p10", "cycles_and_lone_k5_p10")):
        t, k = fresh(ya, synth, name)
        try:
            with yw.Walk(t, 1) as w, yg.Gfa(w, k) as g, yb.Bubbles(w, g, k) as b:
                before = (yw.tally(), yg.tally(), yb.tally(), main_tally(ya))
                with yc.Clean(w, g, b, k):
                    pass
                assert (yw.tally(), yg.tally(), yb.tally(), main_tally(ya)) == before
            assert set(yc.tally().values()) == {i + 1}, yc.tally()
            with yw.Walk(t, 1023) as w, yg.Gfa(w, k) as g, yb.Bubbles(w, g, k) as b, yc.Clean(w, g, b, k) as cl:      # no unitig: no launch
                assert cl.stats() == NOTHING and len(cl.records()) == 0 and cl.image() == b""
            assert set(yc.tally().values()) == {i + 1}
        finally:
            t.close()


def main_tally(ya):
    names = C.POINTER(C.c_char_p)()
    n = ya.lib().yakamd_tally_names(C.byref(names))
    out = (C.c_uint64 * n)()
    ya.lib().yakamd_tally_read(out, n)
    return {names[i].decode(): int(out[i]) for i in range(n)}
