"""`yak-amd paths` on the device (the kernels of yak_amd/path/path.hip behind yakamd_path_open, yakamd_path_hits_dev, yakamd_path_chain_dev,
yakamd_paths, the CLI and yak_amd.path) against the restatements of tests/path_util.py (held to each other, to hand-derived cases and to the
sequential model of the kernels by tests/test_path.py and tests/test_path_model.py), always on the dump of the very table that was walked: the hits
element by element, the path records, the steps and the tallies field by field, both texts byte for byte.  Tables of every degree, of one unitig, of
bubbles across sub-tables, of cycles, without a node, and of every 7-mer -- also with the index at its smallest capacity; sequence ends at every
offset around a tile edge, more tiles than the scan has threads, the empty image, the counting calls, what lies behind the outputs, the refusals,
and a launch of every kernel of the library."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import gfa_util as G
import graph_util as U
import path_util as P
import walk_util as W
from test_gpu_gfa import SHAPES, genome, snp_copies
from test_gpu_graph import CLI, Tab, restated_file

pytestmark = pytest.mark.gpu
PAD = 4096


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the paths have no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def yw(ya):
    import yak_amd.walk
    yak_amd.walk.lib()
    return yak_amd.walk


@pytest.fixture(scope="module")
def yp(yw):
    import yak_amd.path
    yak_amd.path.lib()
    return yak_amd.path


@pytest.fixture(scope="module")
def tabs(ya, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("path")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](synth), int(k[1:]), int(pre[1:]))
            tab.path_want = {}
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def want_of(tab, min_cnt):
    """(records, unitigs, map, links) of the dump, computed once"""
    if min_cnt not in tab.path_want:
        recs, st, ug = tab.restated(min_cnt)
        amap, desc, bases = W.restate(tab.k, recs, min_cnt, ug)
        tab.path_want[min_cnt] = (recs, ug, amap, G.links_by_strings(tab.k, ug))
    return tab.path_want[min_cnt]


def restate(tab, min_cnt, seqs, by_strings=True):
    """what the restatement says of the sequences (bytes) on the table: computed once per test and shared by its device checks"""
    recs, ug, amap, links = want_of(tab, min_cnt)
    img, off, lens = P.image(seqs)
    hits = P.hits_by_ints(tab.k, recs, min_cnt, amap, img)
    if by_strings:
        assert hits == P.hits_by_strings(tab.k, ug, img)
    paths, steps, tally, spans = P.chain(tab.k, ug, hits, off, lens)
    P.check_rules(tab.k, ug, paths, steps, spans, links)
    return dict(img=img, off=off, lens=lens, ug=ug, hits=hits, paths=paths, steps=steps, tally=tally)


def equal(r, hits, paths, steps, tally):
    assert np.array_equal(hits, np.array(r["hits"], np.uint64)), np.flatnonzero(hits != np.array(r["hits"], np.uint64))[:8]
    assert len(paths) == len(r["paths"]) and len(steps) == len(r["steps"])
    for f in ("seq", "qs", "qe", "ps", "step_off", "n_step"):
        want = np.array([p[f] for p in r["paths"]], np.uint64)
        assert np.array_equal(paths[f].astype(np.uint64), want), (f, np.flatnonzero(paths[f].astype(np.uint64) != want)[:8])
    assert np.array_equal(steps, np.array(r["steps"], np.uint64))
    for x, f in enumerate(("n_kmer", "n_hit", "n_path", "n_step")):
        assert np.array_equal(tally[f], np.array([t[x] for t in r["tally"]], np.uint32)), f


def check(yw, yp, tab, min_cnt, seqs, by_strings=True):
    r = restate(tab, min_cnt, seqs, by_strings)
    with yw.Walk(tab.t, min_cnt) as w, yp.Path(w, tab.k) as px:
        hits = px.hits(r["img"])
        paths, steps, tally = px.chain(r["img"], r["off"], r["lens"])
        st = px.stats()
    equal(r, hits, paths, steps, tally)
    n_node = sum(u[1] for u in r["ug"])
    assert (st["n_unitig"], st["n_node"]) == (len(r["ug"]), n_node) and st["max_probe"] <= st["table_slots"]
    if r["ug"]:
        assert st["table_slots"] & (st["table_slots"] - 1) == 0 and st["table_slots"] >= n_node
    return r, st


def both_strands(seqs):
    return [s for q in seqs for s in (q, P.rc_bytes(q))]


def test_every_degree_at_k5(yw, yp, tabs):
    rng = random.Random(5)
    src = [ln for ln in SHAPES["mixed_k5_p10"](None).split(b"\n") if ln]
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(5, 40))).encode() for _ in range(60)] + both_strands(src)
    for min_cnt in (1, 2):
        r, st = check(yw, yp, tabs("mixed_k5_p10"), min_cnt, seqs)
        assert any(p["n_step"] >= 2 for p in r["paths"]) and any(s & 1 for s in r["steps"]) and any(t[2] >= 2 for t in r["tally"])
    assert st["table_slots"] >= 2 * st["n_node"]


def test_reads_on_one_unitig(yw, yp, tabs):
    rng = random.Random(31)
    g = genome(3000, 31).decode()
    seqs = P.reads_of(rng, [g], 300, 100, 100, sub=0.02, n_rate=0.002, mixed_case=True)
    r, st = check(yw, yp, tabs("genome3000_k31_p10"), 1, seqs)
    assert st["n_unitig"] == 1 and len(r["paths"]) > 300 and any(s & 1 for s in r["steps"]) and any(p["ps"] for p in r["paths"])


def test_a_genome_across_69_tiles(yw, yp, tabs):
    """the whole genome as one sequence: one path of eleven steps -- six pieces and an arm of each of the five bubbles; the other arms and their
    reverse complements beside it"""
    recs = [ln for ln in snp_copies().split(b"\n") if ln]
    arms = [a[70:131] for a in recs[1:]]                         # ten k-mers of the flank, the arm's 21, ten of the other flank
    r, st = check(yw, yp, tabs("snps70000_k21_p13"), 1, [recs[0]] + both_strands(arms), by_strings=False)
    assert r["paths"][0]["n_step"] == 11 and r["paths"][0]["qe"] == 70000 and len(r["img"]) > 68 * yp.TILE
    assert all(p["n_step"] == 3 for p in r["paths"][1:]) and len(r["paths"]) == 11


def test_more_tiles_than_the_scan_has_threads(yw, yp, tabs):
    g = [ln for ln in snp_copies().split(b"\n") if ln][0]
    r, st = check(yw, yp, tabs("snps70000_k21_p13"), 1, [g, P.rc_bytes(g)] * 2, by_strings=False)
    assert len(r["img"]) > 256 * yp.TILE and [p["n_step"] for p in r["paths"]] == [11] * 4 and r["paths"][3]["step_off"] == 33


def test_cycles(yw, yp, tabs):
    r, st = check(yw, yp, tabs("cycles_k31_p10"), 1, [b"AC" * 40, b"ACG" * 30, b"GT" * 40])
    n_ac, n_acg = 2, 3                                            # the nodes of the two cycles
    assert [p["n_step"] for p in r["paths"]] == [(80 - 30 + n_ac - 1) // n_ac, (90 - 30 + n_acg - 1) // n_acg, (80 - 30 + n_ac - 1) // n_ac]
    assert len(set(r["steps"][:25])) == 1 and r["steps"][-1] & 1
    r, st = check(yw, yp, tabs("ac8_k5_p10"), 1, [b"AC" * 8, b"ACACAGT"])
    assert st["n_unitig"] == 1 and r["tally"][0] == (12, 12, 1, 6) and r["tally"][1] == (3, 1, 1, 1)


def test_a_table_without_a_node(yw, yp, tabs):
    r, st = check(yw, yp, tabs("ac8_k5_p10"), 1023, [b"AC" * 8, b"ACGTAN", b""])
    assert st == dict(n_unitig=0, n_node=0, table_slots=0, max_probe=0) and r["tally"] == [(12, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0)]
    assert set(r["hits"]) == {P.NONE, P.ABSENT}


def test_every_7_mer(yw, yp, tabs, monkeypatch):
    """8192 unitigs of one node: every k-mer of every sequence is a hit and a step; then 8192 keys in 8192 slots: no free slot is left"""
    rng = random.Random(7)
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(7, 300))).encode() for _ in range(50)]
    tab = tabs("every_k7_p10")
    r, st = check(yw, yp, tab, 1, seqs)
    assert st["n_node"] == 8192 and st["table_slots"] == 16384 and all(t[0] == t[1] == t[3] for t in r["tally"])
    monkeypatch.setenv("YAKAMD_PATH_SLOTS", "8192")
    r, full = check(yw, yp, tab, 1, seqs)
    assert full["table_slots"] == 8192 and full["max_probe"] > st["max_probe"]
    monkeypatch.setenv("YAKAMD_PATH_SLOTS", "8191")
    with yw.Walk(tab.t, 1) as w:
        assert yp.lib().yakamd_path_open(w.w, 7) is None and b"YAKAMD_PATH_SLOTS = 8191: the index has 8192 keys" in yp.lib().yakamd_path_last_error()


def test_sequence_ends_around_a_tile_edge(yw, yp, tabs):
    """the newline of sequence s stands at (s + 1) T + d for every d from -k - 1 to k + 1: paths that end, and paths that begin, at every offset
    around an edge"""
    k, T = 31, yp.TILE
    rng = random.Random(3)
    g = genome(3000, 31)
    seqs, pos = [], 0
    for s, d in enumerate(range(-k - 1, k + 2)):
        ln = (s + 1) * T + d - pos
        a = rng.randint(0, len(g) - ln)
        seqs.append(g[a:a + ln] if s % 2 else P.rc_bytes(g[a:a + ln]))
        pos += ln + 1
    r, st = check(yw, yp, tabs("genome3000_k31_p10"), 1, seqs)
    assert [r["img"].index(b"\n", (s + 1) * T - k - 2) - (s + 1) * T for s in range(2 * k + 3)] == list(range(-k - 1, k + 2))
    assert len(r["paths"]) == 2 * k + 3


def raw_chain(ya, yp, px, r, cap_paths, cap_steps, give=True):
    """yakamd_path_chain_dev on buffers of the caller's with PAD poisoned bytes behind each: (return value, n_out, the raw buffers)"""
    L, M = yp.lib(), ya.lib()
    n, n_seq = len(r["img"]), len(r["off"])
    off, lens = np.array(r["off"], np.uint64), np.array(r["lens"], np.uint32)
    n_path, n_step = len(r["paths"]), len(r["steps"])
    with yp._Dev(M) as dev:
        d_hit, n16 = px._hits_dev(dev, r["img"])
        sizes = dict(paths=n_path * 32, steps=n_step * 8, tally=n_seq * 16)
        bufs = {f: dev.alloc(b + PAD, b"\xa5" * (b + PAD)) for f, b in sizes.items()}
        d_off, d_len = dev.alloc(n_seq * 8, off.tobytes()), dev.alloc(n_seq * 4, lens.tobytes())
        n_out = (C.c_int64 * 2)()
        rc = L.yakamd_path_chain_dev(px.px, d_hit, n, d_off, d_len, n_seq, bufs["paths"] if give else None, cap_paths, bufs["steps"] if give else None, cap_steps,
                                     bufs["tally"], n_out)
        raw = {f: dev.fetch(bufs[f], np.zeros(b + PAD, np.uint8)).tobytes() for f, b in sizes.items()}
    return rc, list(n_out), raw, sizes


def test_counting_calls_and_what_lies_behind_the_outputs(ya, yw, yp, tabs):
    rng = random.Random(11)
    g = genome(3000, 31).decode()
    tab = tabs("genome3000_k31_p10")
    seqs = P.reads_of(rng, [g], 40, 60, 200, sub=0.02, n_rate=0.002)
    if sum(len(s) + 1 for s in seqs) % 16 == 0:                  # the image is to end inside a group of 16
        seqs.append(b"A")
    r = restate(tab, 1, seqs)
    n_path, n_step = len(r["paths"]), len(r["steps"])
    assert n_path > 20 and n_step >= n_path
    poison = lambda b: b"\xa5" * b
    with yw.Walk(tab.t, 1) as w, yp.Path(w, 31) as px:
        hits = px.hits(r["img"])
        rc, n_out, raw, sizes = raw_chain(ya, yp, px, r, n_path, n_step)
        assert rc == 0 and n_out == [n_path, n_step]
        for f, b in sizes.items():
            assert raw[f][b:] == poison(PAD), "written behind the " + f
        paths, steps = np.frombuffer(raw["paths"][:sizes["paths"]], yp.PATH_DTYPE), np.frombuffer(raw["steps"][:sizes["steps"]], np.uint64)
        tally = np.frombuffer(raw["tally"][:sizes["tally"]], yp.TALLY_DTYPE)
        equal(r, hits, paths, steps, tally)
        for cp, cs, give in ((n_path - 1, n_step, True), (n_path, n_step - 1, True), (0, 0, True), (n_path, n_step, False)):
            rc, n_out, raw2, _ = raw_chain(ya, yp, px, r, cp, cs, give)
            assert rc == 1 and n_out == [n_path, n_step], (cp, cs, give)
            assert raw2["paths"] == poison(sizes["paths"] + PAD) and raw2["steps"] == poison(sizes["steps"] + PAD), "a counting call wrote a record"
            assert raw2["tally"] == raw["tally"]
        # the hits: n rounded up to 16 entries and nothing behind them
        n, M = len(r["img"]), ya.lib()
        n16 = (n + 15) & ~15
        assert n % 16
        with yp._Dev(M) as dev:
            d_img = dev.alloc(n16, r["img"] + b"A" * (n16 - n))       # bases behind the image are not looked at
            d_hit = dev.alloc(n16 * 8 + PAD, poison(n16 * 8 + PAD))
            assert px.L.yakamd_path_hits_dev(px.px, d_img, n, d_hit) == 0
            got = dev.fetch(d_hit, np.zeros(n16 * 8 + PAD, np.uint8)).tobytes()
        assert got[n16 * 8:] == poison(PAD) and np.array_equal(np.frombuffer(got[:n * 8], np.uint64), hits)
        assert set(np.frombuffer(got[n * 8:n16 * 8], np.uint64).tolist()) == {P.NONE}


def test_the_empty_image_launches_nothing(ya, yw, yp, tabs):
    tab = tabs("ac8_k5_p10")
    with yw.Walk(tab.t, 1) as w, yp.Path(w, 5) as px:
        yp.lib().yakamd_path_tally_reset()
        assert len(px.hits(b"")) == 0
        paths, steps, tally = px.chain(b"", [], [])
        assert len(paths) == len(steps) == len(tally) == 0
        n_out = (C.c_int64 * 2)(7, 7)
        assert px.L.yakamd_path_chain_dev(px.px, None, 0, None, None, 0, None, 0, None, 0, None, n_out) == 0 and list(n_out) == [0, 0]
        assert not any(yp.tally().values())


def test_the_index_outlives_the_walk(yw, yp, tabs):
    tab = tabs("mixed_k5_p10")
    r = restate(tab, 1, [b"ACGTACGTTGCAAACCC", b"AAAAAAAA"])
    w = yw.Walk(tab.t, 1)
    px = yp.Path(w, 5)
    w.close()
    try:
        equal(r, px.hits(r["img"]), *px.chain(r["img"], r["off"], r["lens"]))
    finally:
        px.close()


def call_text(yp, h, fn, out, **kw):
    o = yp.PpoptT()
    yp.lib().yakamd_ppopt_init(C.byref(o))
    for f, v in kw.items():
        setattr(o, f, v)
    if os.path.exists(out):
        os.remove(out)
    assert yp.lib().yakamd_paths(C.byref(o), h, fn.encode(), out.encode()) == 0, yp._err()
    return open(out, "rb").read()


def test_command_texts(ya, yw, yp, tabs, tmp_path):
    """yakamd_paths on the resident table; the CLI and yak_amd.path on its file (the listing order, and with it the numbering, is the restored
    table's)"""
    rng = random.Random(8)
    tab = tabs("mixed_k5_p10")
    src = [ln.decode() for ln in SHAPES["mixed_k5_p10"](None).split(b"\n") if ln]
    seqs = P.reads_of(rng, src[:1], 40, 3, 60, sub=0.05, n_rate=0.02, mixed_case=True) + [b""]
    names = ["r%d" % i for i in range(len(seqs))]
    fa, out = str(tmp_path / "s.fa"), str(tmp_path / "o.gaf")
    open(fa, "wb").write(b"".join(b">%s some words\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    for min_cnt in (1, 2):
        r = restate(tab, min_cnt, seqs)
        gaf, stats = P.gaf_text(5, r["ug"], names, r["lens"], r["paths"], r["steps"]), P.stats_text(5, min_cnt, names, r["lens"], r["tally"])
        assert min_cnt > 1 or gaf.count(b"\n") > 30
        for chunk in (1, 1000, 1 << 28):
            assert call_text(yp, tab.t.h, fa, out, min_cnt=min_cnt, chunk_size=chunk) == gaf
            assert call_text(yp, tab.t.h, fa, out, min_cnt=min_cnt, chunk_size=chunk, stats_only=1) == stats
        assert call_text(yp, tab.t.h, fa, out, min_cnt=min_cnt, min_len=5) == gaf
        few = P.gaf_text(5, r["ug"], names, r["lens"], r["paths"], r["steps"], min_len=20)
        assert min_cnt > 1 or 0 < few.count(b"\n") < gaf.count(b"\n")
        assert call_text(yp, tab.t.h, fa, out, min_cnt=min_cnt, min_len=20) == few
    with gzip.open(fa + ".gz", "wb") as f:
        f.write(open(fa, "rb").read())
    assert call_text(yp, tab.t.h, fa + ".gz", out, min_cnt=2) == gaf
    # the file's table
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
    finally:
        back.close()
    run = lambda a: subprocess.run([CLI, "paths"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    k, recs, st, ug = restated_file(f, 1)
    amap, desc, bases = W.restate(k, recs, 1, ug)
    img, off, lens = P.image(seqs)
    paths, steps, tally, spans = P.chain(k, ug, P.hits_by_ints(k, recs, 1, amap, img), off, lens)
    gaf, stats = P.gaf_text(k, ug, names, lens, paths, steps), P.stats_text(k, 1, names, lens, tally)
    assert run([tab.fn, fa]) == gaf == yp.paths(tab.fn, fa) == run(["-K", "1", tab.fn, fa]) == run(["-K1000", tab.fn, fa + ".gz"])
    assert run(["-s", tab.fn, fa]) == stats == yp.paths(tab.fn, fa, stats_only=True, chunk_size=1)
    assert run(["-l", "20", "-o", out, tab.fn, fa]) == b"" and open(out, "rb").read() == P.gaf_text(k, ug, names, lens, paths, steps, min_len=20) == yp.paths(tab.fn, fa, min_len=20)
    segs = {ln.split(b"\t")[1] for ln in subprocess.run([CLI, "unitigs", "-G", tab.fn], check=True, stdout=subprocess.PIPE, timeout=600).stdout.split(b"\n") if ln[:1] == b"S"}
    used = {w[1:] for ln in gaf.split(b"\n") if ln for w in ln.split(b"\t")[5].replace(b"<", b" <").replace(b">", b" >").split()}
    assert used and used <= segs
    for a in (["-c", "0", "-o", out + "2", tab.fn, fa], ["-l", "-1", "-o", out + "2", tab.fn, fa], ["-o", out + "2", tab.fn, fa + ".none"], ["-o", out + "2", tab.fn]):
        q = subprocess.run([CLI, "paths"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert q.returncode != 0 and q.stdout == b"" and q.stderr and not os.path.exists(out + "2"), a
    q = subprocess.run([CLI, "paths", "-o", out + "2", tab.fn, fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, YAKAMD_PATH_SLOTS="1"))
    assert q.returncode == 3 and b"YAKAMD_PATH_SLOTS = 1" in q.stderr and not os.path.exists(out + "2")


def test_refusals(ya, yw, yp, tabs, synth, tmp_path, monkeypatch):
    L = yp.lib()
    out, fa = str(tmp_path / "o.gaf"), str(tmp_path / "s.fa")
    open(fa, "wb").write(b">r\nACGTACGTACGT\n")
    tab = tabs("genome3000_k31_p10")
    with yw.Walk(tab.t, 1) as w:
        for k, what in ((30, b"odd"), (2, b"odd"), (1, b"[3, 31]"), (33, b"[3, 31]"), (-5, b"[3, 31]"), (29, b"does not fit the walk"), (21, b"does not fit the walk")):
            assert L.yakamd_path_open(w.w, k) is None and what in L.yakamd_path_last_error(), (k, L.yakamd_path_last_error())
        monkeypatch.setenv("YAKAMD_PATH_MAX_BYTES", "100000")
        need = 16 * 8192 + 32 + 3008                               # 2970 nodes in 8192 slots, one descriptor, 3000 bases rounded up to 16
        assert L.yakamd_path_open(w.w, 31) is None and (b"%d bytes of device memory are needed" % need) in L.yakamd_path_last_error()
        monkeypatch.setenv("YAKAMD_PATH_MAX_BYTES", str(need))
        with yp.Path(w, 31) as px:
            st = yp.PxstatT()
            assert L.yakamd_path_stats(px.px, None) == -1 and L.yakamd_path_stats(None, C.byref(st)) == -1
            d = ya.lib().yakamd_dev_alloc(4096)
            try:
                n_out = (C.c_int64 * 2)()
                assert L.yakamd_path_hits_dev(px.px, d + 8, 100, d + 1024) == -1 and b"aligned" in L.yakamd_path_last_error()
                assert L.yakamd_path_hits_dev(px.px, d, -1, d + 1024) == -1
                assert L.yakamd_path_chain_dev(px.px, d + 8, 100, d, d, 1, None, 0, None, 0, None, n_out) == -1 and b"aligned" in L.yakamd_path_last_error()
                assert L.yakamd_path_chain_dev(px.px, d, 100, None, None, 1, None, 0, None, 0, None, n_out) == -1
                assert L.yakamd_path_chain_dev(px.px, d, 100, None, None, 0, None, 0, None, 0, None, n_out) == -1 and b"in no sequence" in L.yakamd_path_last_error()
            finally:
                ya.lib().yakamd_dev_free(d)
        monkeypatch.delenv("YAKAMD_PATH_MAX_BYTES")
    with yw.Walk(tab.t, 1023) as w, yp.Path(w, 5) as px:                # a walk without unitigs fits every k and opens
        assert px.stats()["n_unitig"] == 0
    o = yp.PpoptT()
    L.yakamd_ppopt_init(C.byref(o))
    for h, min_cnt, min_len, fn, what in ((None, 1, 0, fa, b"not an engine table"), (tab.t.h, 0, 0, fa, b"min_cnt 0"), (tab.t.h, 1024, 0, fa, b"min_cnt 1024"),
                                          (tab.t.h, 1, -1, fa, b"min_len -1"), (tab.t.h, 1, 0, fa + ".none", b"cannot read")):
        o.min_cnt, o.min_len = min_cnt, min_len
        assert L.yakamd_paths(C.byref(o), h, fn.encode(), out.encode()) == -1 and what in L.yakamd_path_last_error(), (what, L.yakamd_path_last_error())
        assert not os.path.exists(out), "a refused call created its output"
    o.min_cnt, o.min_len = 1, 0
    monkeypatch.setenv("YAKAMD_WALK_MAX_BYTES", "1")
    assert L.yakamd_paths(C.byref(o), tab.t.h, fa.encode(), out.encode()) == -1 and b"walk:" in L.yakamd_path_last_error() and not os.path.exists(out)
    monkeypatch.delenv("YAKAMD_WALK_MAX_BYTES")
    for k, mark, what in ((30, 0, b"even"), (31, 1, b"homopolymer-compressed")):
        t = ya.Table(k, 10, 4, 0)
        try:
            if mark:
                assert ya.lib().yakamd_ch_set_hpc(t.h, 1) == 0
            t.count_pass_host(1, synth(300, 150, 2500, s=5))
            assert L.yakamd_paths(C.byref(o), t.h, fa.encode(), out.encode()) == -1 and what in L.yakamd_path_last_error() and not os.path.exists(out)
        finally:
            t.close()


def test_every_kernel_is_launched(ya, yw, yp, tabs):
    """the six kernels of the library's tally and no other launch: the open launches the index once, a call for hits the hits, a counting call the
    count, the scan and, given a place for them, the tallies; a writing call the count, the scan and the emit"""
    assert set(yp.tally()) == {"k_path_index", "k_path_hits", "k_path_count", "k_path_tile_scan", "k_path_tally", "k_path_emit"}
    tab = tabs("mixed_k5_p10")
    r = restate(tab, 1, [b"ACGTACGTTGCAAACCC", b"AAAAAAAA"])
    yp.lib().yakamd_path_tally_reset()
    zero = dict.fromkeys(yp.tally(), 0)
    with yw.Walk(tab.t, 1) as w:
        before_walk = yw.tally()
        with yp.Path(w, 5) as px:
            assert yp.tally() == dict(zero, k_path_index=1) and yw.tally() == before_walk      # the index launches nothing of the walk's
            px.hits(r["img"])
            assert yp.tally() == dict(zero, k_path_index=1, k_path_hits=1)
            px.chain(r["img"], r["off"], r["lens"])                # hits, a counting call with tallies, a writing call without
            assert yp.tally() == dict(k_path_index=1, k_path_hits=2, k_path_count=2, k_path_tile_scan=2, k_path_tally=1, k_path_emit=1)
    with yw.Walk(tab.t, 1023) as w, yp.Path(w, 5) as px:               # no unitig: no index to build, and no path to write
        px.chain(r["img"], r["off"], r["lens"])
    assert yp.tally() == dict(k_path_index=1, k_path_hits=3, k_path_count=3, k_path_tile_scan=3, k_path_tally=2, k_path_emit=1)
