"""The read support of the bubbles' alleles on the device (the kernels of yak_amd/allele/allele.hip behind yakamd_allele_open, yakamd_allele_obs_dev,
yakamd_allele_support_dev, yakamd_alleles, the CLI's `bubbles -r` and yak_amd.allele) against the restatement of tests/allele_util.py (held to a
second one, to hand-derived cases and to the sequential model of the kernels by tests/test_allele.py and tests/test_allele_model.py), always on
the dump of the very table that was walked: the records one by one, the support, the texts byte for byte.  The shapes are the smallest that can
go wrong: an observation as the last step of a workgroup's 256 and as the first of the next, and of a tile of the scan; paths across those edges
and a path that holds whole workgroups; more tiles than the scan kernel has threads; two calls that add up, a counting call that adds nothing, a
reset; 4 KiB behind every output; no step and no bubble; the texts in three chunk sizes from FASTA, FASTQ and gzip with -s, -f, -m and -n;
damaged inputs, each caught by a bound check that the model has exercised on the CPU; the refusals; a launch of every kernel; and `bubbles`
without -r, which is what it was."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import allele_util as A
import bubble_util as B
import graph_util as U
import path_util as P
from test_allele import KERNELS, TWO
from test_bubble import CIRCLE, HAND, PLANTED_SEEDS
from test_gpu_bubble import many_snps
from test_gpu_graph import CLI, Tab, restated_file

pytestmark = pytest.mark.gpu
T = 600
PAD = 4096
WG, TILE = 256, 1024                           # the steps of a workgroup of k_al_find, and of a tile of the scan


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the alleles have no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def libs(ya):
    import yak_amd.allele
    import yak_amd.bubble
    import yak_amd.gfa
    import yak_amd.path
    import yak_amd.walk
    yak_amd.allele.lib()
    return yak_amd.walk, yak_amd.gfa, yak_amd.bubble, yak_amd.path, yak_amd.allele


def hand_image(name):
    return lambda: U.image([s.encode() for s in (HAND[name][1] if name in HAND else TWO)])


SHAPES = {
    "bubble_k5_p10": hand_image("bubble"), "twosnps_k5_p10": hand_image("two_snps"), "circle_k5_p10": hand_image("circle"), "two_k5_p10": hand_image("two"),
    "tip_k5_p10": hand_image("tip"), "closing_k5_p10": hand_image("closing"),
    "planted_k31_p13": lambda: U.image([s.encode() for s in B.planted(31, 1000, PLANTED_SEEDS[(31, False)])[0]]),
    "manysnps_k15_p10": lambda: many_snps(15, 6000, 15),
}


@pytest.fixture(scope="module")
def tabs(ya, tmp_path_factory):
    d = tmp_path_factory.mktemp("allele")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](), int(k[1:]), int(pre[1:]))
            tab.al_want = {}
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def want_of(tab, min_cnt=1):
    """(unitigs, bubble records) of the dump, computed once"""
    if min_cnt not in tab.al_want:
        recs, st, ug = tab.restated(min_cnt)
        bub, bs = B.by_strings(tab.k, ug)
        tab.al_want[min_cnt] = (ug, bub)
    return tab.al_want[min_cnt]


class Opened:
    """the walk, the links, the bubbles, the arm map and the index of a table, the first three closed once the last two stand"""

    def __init__(self, libs, tab, min_cnt=1, path=True):
        yw, yg, yb, yp, yl = libs
        with yw.Walk(tab.t, min_cnt) as w, yg.Gfa(w, tab.k) as g, yb.Bubbles(w, g, tab.k) as b:
            self.al = yl.Alleles(w, b)
            self.px = yp.Path(w, tab.k) if path else None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.al.close()
        if self.px:
            self.px.close()


def as_paths(paths):
    return np.array([(p["step_off"], p["ps"], p["seq"], p["n_step"], p["qs"], p["qe"]) for p in paths], P_DTYPE)


P_DTYPE = np.dtype([("step_off", "<u8"), ("ps", "<u8"), ("seq", "<u4"), ("n_step", "<u4"), ("qs", "<u4"), ("qe", "<u4")])


def rows(obs):
    return [(int(o["seq"]), int(o["bubble"]), int(o["flags"]), int(o["path"])) for o in obs]


def sup_rows(sup):
    return [(int(s["full"][0]), int(s["full"][1]), int(s["part"][0]), int(s["part"][1])) for s in sup]


def check(libs, tab, reads, min_cnt=1):
    """the reads through the index, the chain and the observations of the device against flat() on the dump"""
    ug, recs = want_of(tab, min_cnt)
    d = A.flat(tab.k, ug, recs, reads)
    A.check_invariants(recs, d)
    img, off, lens = P.image(reads)
    with Opened(libs, tab, min_cnt) as o:
        assert o.al.stats() == dict(n_unitig=len(ug), n_bubble=len(recs), n_arm=2 * len(recs))
        paths, steps, tally = o.px.chain(img, off, lens)
        assert [int(s) for s in steps] == d["steps"] and [int(p["step_off"]) for p in paths] == [p["step_off"] for p in d["paths"]]
        obs, n_obs, n_full = o.al.observe(paths, steps)
        print("obs", n_obs, n_full, "ms", libs[4].ms())
        assert rows(obs) == d["obs"] and (n_obs, n_full) == (len(d["obs"]), sum(1 for x in d["obs"] if x[2] & A.FULL))
        assert sup_rows(o.al.support()) == d["sup"]
    return d


def test_hand_cases_at_k5(libs, tabs):
    read = CIRCLE * 2 + CIRCLE[:8]
    cases = {
        "bubble": ["TTCAGGTCTCATG", "TTCAGGACTCATG", "CATGAGACCTGAA", "CATGAGTCCTGAA", "GGTCTCATG", "TTCAGGTCT", "TTCAGGTCNCATG", "TTCAGGNCTCATG", "CTCATG", "TTCA",
                   "ttcaggucucaug"],
        "twosnps": ["CAGAAAATAGCGACGGACC", "CAGAAAATCGCGACGGACC", "CAGAAAATNGCGACGGACC"],
        "circle": [read, U.rc_str(read)],
        "two": [TWO[0], TWO[1], U.rc_str(TWO[0][:14] + TWO[1][14:]), TWO[0][:15], TWO[1][12:]],
        "tip": ["TTCAGGACTCATG", "CAGGAGG"],
    }
    want = dict(bubble=(5, 3), twosnps=(1, 4), circle=(4, 2), two=(8, 0), tip=(0, 0))      # full and partial, as tests/test_allele.py writes them out
    for name, reads in cases.items():
        d = check(libs, tabs(name + "_k5_p10"), [r.encode() for r in reads])
        assert (sum(s[0] + s[1] for s in d["sup"]), sum(s[2] + s[3] for s in d["sup"])) == want[name], name


def test_planted_genome_and_many_snps(libs, tabs):
    rng = random.Random(31)
    haps = B.planted(31, 1000, PLANTED_SEEDS[(31, False)])[0]
    d = check(libs, tabs("planted_k31_p13"), P.reads_of(rng, haps, 60, 62, 400, sub=0.002))
    assert sum(1 for o in d["obs"] if o[2] & A.FULL) > 50 and {o[2] & A.REV for o in d["obs"]} == {0, A.REV}
    img = many_snps(15, 6000, 15)
    d = check(libs, tabs("manysnps_k15_p10"), P.reads_of(rng, [s.decode() for s in img.split(b"\n") if s], 40, 100, 600))
    assert len(d["steps"]) > 2 * WG and len(want_of(tabs("manysnps_k15_p10"))[1]) > 100


# ---- the device-level call on lists of the test's own making ----
def device_obs(ya, al, paths, steps, cap=None, give=True):
    """yakamd_allele_obs_dev on buffers of the caller's with PAD poisoned bytes behind the records: (return value, n_out, the raw record buffer)"""
    from yak_amd.path import _Dev
    n_path, n_step = len(paths), len(steps)
    with _Dev(ya.lib()) as dev:
        d_paths, d_steps = dev.alloc(paths.nbytes, paths.tobytes()), dev.alloc(steps.nbytes, steps.tobytes())
        size = (cap if cap is not None else 0) * 16 + PAD
        d_obs = dev.alloc(size, b"\xa5" * size)
        n_out = (C.c_int64 * 2)(7, 7)
        rc = al.L.yakamd_allele_obs_dev(al.al, d_paths, n_path, d_steps, n_step, d_obs if give else None, cap if cap is not None else 0, n_out)
        raw = dev.fetch(d_obs, np.zeros(size, np.uint8)).tobytes()
    return rc, list(n_out), raw


def lists_of(lengths, step_at):
    """path records of the given numbers of steps, one sequence each, and their steps"""
    paths, at = [], 0
    for s, n in enumerate(lengths):
        paths.append(dict(step_off=at, ps=0, seq=s, n_step=n, qs=0, qe=0))
        at += n
    return paths, [step_at(t) for t in range(at)]


def edge_lists(ug, recs, seed):
    """paths and steps whose observations stand on both sides of every edge: a step on an arm at t = 255, 256, 1023, 1024, ... (last of a workgroup,
    first of the next; of a tile of the scan), paths that end at, begin at and straddle those edges, a path that holds three whole workgroups,
    and random short ones; every other step on an arm with probability 1/4"""
    rng = random.Random(seed)
    arms = [a >> 1 for r in recs for a in r[2]]
    rest = [j for j in range(len(ug)) if j not in arms]
    lengths = [WG - 1, 2, 3 * WG + 5, 1, 1, WG - 7, 3]           # ends at 254; 255-256 straddles; 257 .. 1029 holds workgroups 2 and 3 and the tile edge
    while sum(lengths) < 3 * TILE - 40:
        lengths.append(rng.choice((1, 1, 2, 3, 3, 5, 40)))
    lengths.append(3 * TILE + 1 - sum(lengths))                  # to one step behind the third tile
    forced = {t for e in range(WG, 3 * TILE + 1, WG) for t in (e - 1, e)}
    step_at = lambda t: (rng.choice(arms) if t in forced or rng.random() < 0.25 else rng.choice(rest)) << 1 | rng.randrange(2)
    return lists_of(lengths, step_at)


def test_tile_edges(ya, libs, tabs):
    """an observation as the last step of one workgroup and as the first of the next, of one tile of the scan and of the next; paths that straddle
    an edge, so that the bounded search has a first and a last path that differ; a workgroup wholly inside one path"""
    tab = tabs("two_k5_p10")
    ug, recs = want_of(tab)
    paths, steps = edge_lists(ug, recs, 5)
    assert len(steps) == 3 * TILE + 1
    want, at = A.observe(paths, steps, recs, A.arm_map(len(ug), recs))
    assert {t for e in range(WG, 3 * TILE + 1, WG) for t in (e - 1, e)} <= set(at)
    firsts = [p["step_off"] for p in paths]
    assert any(a < WG <= a + p["n_step"] - 1 for a, p in zip(firsts, paths)) and any(a <= 2 * WG and a + p["n_step"] >= 3 * WG for a, p in zip(firsts, paths))
    assert {o[2] & A.FULL for o in want} == {0, A.FULL}
    ap, st = as_paths(paths), np.array(steps, np.uint64)
    with Opened(libs, tab, path=False) as o:
        obs, n_obs, n_full = o.al.observe(ap, st)
        assert rows(obs) == want and (n_obs, n_full) == (len(want), sum(1 for x in want if x[2] & A.FULL))
        assert sup_rows(o.al.support()) == A.support(len(recs), want)
        # the records end where they end: 4 KiB behind them stay what they were, for the exact room and for more
        for cap in (len(want), len(want) + 9):
            rc, n_out, raw = device_obs(ya, o.al, ap, st, cap)
            assert rc == 0 and n_out == [n_obs, n_full] and raw[len(want) * 16:] == b"\xa5" * (len(raw) - len(want) * 16), "written behind the records"
            assert rows(np.frombuffer(raw[:len(want) * 16], libs[4].OBS_DTYPE)) == want
        assert sup_rows(o.al.support()) == [tuple(3 * x for x in s) for s in A.support(len(recs), want)]      # three writing calls
        # a counting call writes no record and adds nothing
        before = o.al.support()
        for cap, give in ((len(want) - 1, True), (0, True), (len(want), False)):
            rc, n_out, raw = device_obs(ya, o.al, ap, st, cap, give)
            assert rc == 1 and n_out == [n_obs, n_full] and raw == b"\xa5" * len(raw), "a counting call wrote a record"
        assert np.array_equal(o.al.support(), before)
        # the support through a buffer of the caller's
        L, n_b = ya.lib(), len(recs)
        get = o.al.L.yakamd_allele_support_dev
        d = L.yakamd_dev_alloc(n_b * 32 + PAD)
        try:
            poison, raw = b"\xa5" * (n_b * 32 + PAD), C.create_string_buffer(n_b * 32 + PAD)
            assert L.yakamd_memcpy_h2d(d, poison, len(poison)) == 0
            assert get(o.al.al, None, 0) == n_b == get(o.al.al, d, n_b - 1) == get(o.al.al, None, n_b)
            assert L.yakamd_memcpy_d2h(raw, d, len(poison)) == 0 and raw.raw == poison, "a size query wrote"
            assert get(o.al.al, d, n_b + 3) == n_b and L.yakamd_memcpy_d2h(raw, d, len(poison)) == 0
            assert raw.raw[n_b * 32:] == poison[n_b * 32:] and sup_rows(np.frombuffer(raw.raw[:n_b * 32], libs[4].SUP_DTYPE)) == sup_rows(before)
            assert get(o.al.al, d + 8, n_b) == -1 and b"aligned" in o.al.L.yakamd_allele_last_error()
        finally:
            L.yakamd_dev_free(d)
        o.al.reset()
        assert sup_rows(o.al.support()) == [(0, 0, 0, 0)] * n_b
        obs, _, _ = o.al.observe(ap, st)
        assert rows(obs) == want and sup_rows(o.al.support()) == A.support(n_b, want)


def test_more_tiles_than_the_scan_has_threads(ya, libs, tabs, tmp_path):
    """many short reads over the k = 5 bubble: four reads, of which the restatement says what they give, 30 000 times over -- 270 000 steps in 264
    tiles, more than the 256 threads of the scan of the tile sums, so that a thread scans two"""
    tab = tabs("bubble_k5_p10")
    ug, recs = want_of(tab)
    reads = [b"TTCAGGTCTCATG", b"GGTCTCATG", b"CATGAGTCCTGAA", b"CTCATG"]
    d = A.flat(5, ug, recs, reads)
    reps, n_p, n_s, n_o = 30000, len(d["paths"]), len(d["steps"]), len(d["obs"])
    assert (n_p, n_s, n_o) == (4, 9, 3) and reps * n_s > 256 * TILE
    one = as_paths(d["paths"])
    ap = np.tile(one, reps)
    rep = np.repeat(np.arange(reps, dtype=np.uint64), n_p)
    ap["step_off"] += rep * n_s
    ap["seq"] += (rep * len(reads)).astype(np.uint32)
    st = np.tile(np.array(d["steps"], np.uint64), reps)
    with Opened(libs, tab, path=False) as o:
        obs, n_obs, n_full = o.al.observe(ap, st)
        assert (n_obs, n_full) == (reps * n_o, reps * sum(1 for x in d["obs"] if x[2] & A.FULL))
        r = np.repeat(np.arange(reps, dtype=np.uint32), n_o)
        for x, f in enumerate(("seq", "bubble", "flags", "path")):
            want = np.tile(np.array([ob[x] for ob in d["obs"]], np.uint32), reps) + (r * (len(reads) if f == "seq" else n_p if f == "path" else 0))
            assert np.array_equal(obs[f], want), f
        assert sup_rows(o.al.support()) == [tuple(reps * x for x in s) for s in d["sup"]]
    # the same reads through the command, in chunks of about a third
    fa = str(tmp_path / "many.fa")
    with open(fa, "wb") as f:
        f.write(b"".join(b">r%d\n%s\n" % (i, reads[i % 4]) for i in range(4 * reps)))
    text = call_text(libs[4], tab.t.h, fa, str(tmp_path / "o.txt"), chunk_size=400000)
    s = d["sup"][0]
    assert text == ("#alleles\tk=5\tmin_cnt=1\tmin_sup=2\nA\t0\t%s\t%s\t%d\t%d\t%d\t%d\thet\nT\t%d\t%d\t%d\t%d\t%d\t%d\t0\t1\t1\t0\t0\t0\n" % (
        (B.end_name(recs[0][2][0]), B.end_name(recs[0][2][1])) + tuple(reps * x for x in s) + (4 * reps, reps * sum(map(len, reads)), reps * n_p, reps * n_s, reps * n_o,
                                                                                                reps * 2))).encode()


def test_no_step_and_no_bubble(ya, libs, tabs):
    """n_step = 0 launches nothing; a graph without a bubble opens, and nothing is observed or launched"""
    yl = libs[4]
    with Opened(libs, tabs("bubble_k5_p10"), path=False) as o:
        yl.lib().yakamd_allele_tally_reset()
        obs, n_obs, n_full = o.al.observe(np.zeros(0, P_DTYPE), np.zeros(0, np.uint64))
        assert len(obs) == 0 and (n_obs, n_full) == (0, 0)
        n_out = (C.c_int64 * 2)(7, 7)
        assert o.al.L.yakamd_allele_obs_dev(o.al.al, None, 0, None, 0, None, 0, n_out) == 1 and list(n_out) == [0, 0]
        assert not any(yl.tally().values())
    tab = tabs("tip_k5_p10")
    ug, recs = want_of(tab)
    assert recs == []
    with Opened(libs, tab) as o:
        assert o.al.stats() == dict(n_unitig=len(ug), n_bubble=0, n_arm=0) and len(o.al.support()) == 0
        img, off, lens = P.image([b"TTCAGGACTCATG", b"CAGGAGG"])
        paths, steps, _ = o.px.chain(img, off, lens)
        obs, n_obs, n_full = o.al.observe(paths, steps)
        assert len(steps) == 4 and len(obs) == 0 and (n_obs, n_full) == (0, 0)
        assert not any(yl.tally().values())


# ---- the command ----
def call_text(yl, h, fn, out, **kw):
    o = yl.AloptT()
    yl.lib().yakamd_alopt_init(C.byref(o))
    for f, v in kw.items():
        setattr(o, f, v)
    if os.path.exists(out):
        os.remove(out)
    assert yl.lib().yakamd_alleles(C.byref(o), h, fn.encode(), out.encode()) == 0, yl._err()
    return open(out, "rb").read()


def test_command_texts(ya, libs, tabs, tmp_path):
    """yakamd_alleles on the resident table in three chunk sizes from FASTA, FASTQ and gzip, with -s, -f, -m and -n; the CLI and yak_amd.allele on
    its file (the listing order, and with it the numbering, is the restored table's); `bubbles` without -r is what yakamd_bubbles writes"""
    yw, yg, yb, yp, yl = libs
    rng = random.Random(8)
    tab = tabs("manysnps_k15_p10")
    src = [s.decode() for s in many_snps(15, 6000, 15).split(b"\n") if s]
    reads = P.reads_of(rng, src, 150, 10, 500, sub=0.003, n_rate=0.001, mixed_case=True) + [b""]
    names = ["r%d" % i for i in range(len(reads))]
    fa, fq, out = str(tmp_path / "s.fa"), str(tmp_path / "s.fq"), str(tmp_path / "o.txt")
    open(fa, "wb").write(b"".join(b">%s some words\n%s\n" % (n.encode(), s) for n, s in zip(names, reads)))
    open(fq, "wb").write(b"".join(b"@%s\n%s\n+\n%s\n" % (n.encode(), s, b"I" * len(s)) for n, s in zip(names, reads)))
    with gzip.open(fa + ".gz", "wb") as f:
        f.write(open(fa, "rb").read())
    ug, recs = want_of(tab)
    d = A.flat(15, ug, recs, reads)
    text = lambda **kw: A.text(15, 1, kw.get("min_sup", 2), kw.get("min_frag", 1), kw.get("fragments", 0), kw.get("stats_only", 0), names, recs, d)
    assert text(fragments=1).count(b"\nF\t") > 20 and 0 < text(fragments=1, min_frag=3).count(b"\nF\t") < text(fragments=1).count(b"\nF\t")
    assert len({A.call(s, 2) for s in d["sup"]}) == 4 and text(min_sup=1) != text() != text(min_sup=3)
    for fn in (fa, fq, fa + ".gz"):
        for chunk in (1, 3000, 1 << 28):
            assert call_text(yl, tab.t.h, fn, out, chunk_size=chunk, fragments=1) == text(fragments=1), (fn, chunk)
            assert call_text(yl, tab.t.h, fn, out, chunk_size=chunk) == text()
            assert call_text(yl, tab.t.h, fn, out, chunk_size=chunk, stats_only=1, fragments=1) == text(stats_only=1, fragments=1)
    for kw in (dict(min_sup=1), dict(min_sup=3, fragments=1), dict(min_frag=3, fragments=1), dict(stats_only=1), dict(min_frag=3)):
        assert call_text(yl, tab.t.h, fa, out, **kw) == text(**kw), kw
    ug2, recs2 = want_of(tab, 2)                                   # every node was seen once or twice: nothing forks at 2
    assert recs2 == [] and call_text(yl, tab.t.h, fa, out, min_cnt=2).startswith(b"#alleles\tk=15\tmin_cnt=2\tmin_sup=2\nT\t151\t")
    # the file's table
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
        plain = {s: bubbles_text(ya, yb, back.h, str(tmp_path / "b.txt"), s) for s in (False, True)}
    finally:
        back.close()
    k, _, st, ugf = restated_file(f, 1)
    recsf = B.by_strings(k, ugf)[0]
    df = A.flat(k, ugf, recsf, reads)
    text = lambda **kw: A.text(15, 1, kw.get("min_sup", 2), kw.get("min_frag", 1), kw.get("fragments", 0), kw.get("stats_only", 0), names, recsf, df)
    run = lambda a: subprocess.run([CLI, "bubbles"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=T).stdout
    assert run(["-r", fa, tab.fn]) == text() == yl.alleles(tab.fn, fa) == yl.alleles(tab.fn, fq, chunk_size=1)
    assert run(["-r", fq, "-f", tab.fn]) == text(fragments=1) == yl.alleles(tab.fn, fa + ".gz", fragments=True)
    assert run(["-f", "-n3", "-m", "3", "-r", fa + ".gz", tab.fn]) == text(fragments=1, min_frag=3, min_sup=3) == yl.alleles(tab.fn, fa, fragments=True, min_frag=3, min_sup=3)
    assert run(["-s", "-r", fa, tab.fn]) == text(stats_only=1) == yl.alleles(tab.fn, fa, stats_only=True)
    assert run(["-r", fa, "-o", out + "2", tab.fn]) == b"" and open(out + "2", "rb").read() == text()
    # the i of an A line and its arms are those of the B line of `bubbles`
    blines = [ln.split("\t") for ln in run([tab.fn]).decode().splitlines()[1:]]
    alines = [ln.split("\t") for ln in text().decode().splitlines() if ln[0] == "A"]
    assert len(alines) == len(blines) > 100 and all(a[1] == b[1] and a[2:4] == b[3:5] for a, b in zip(alines, blines))
    # without -r: what it was
    assert run([tab.fn]) == plain[False] == B.text(k, 1, ugf, recsf) and run(["-s", tab.fn]) == plain[True]
    os.remove(out + "2")
    for a in (["-r", fa + ".none"], ["-r", fa, "-m", "0"], ["-r", fa, "-n", "0"], ["-r", fa, "-c", "0"], ["-m", "2"], ["-f"]):
        q = subprocess.run([CLI, "bubbles", "-o", out + "2"] + a + [tab.fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
        assert q.returncode != 0 and q.stdout == b"" and q.stderr and not os.path.exists(out + "2"), a


def bubbles_text(ya, yb, h, out, stats):
    from test_gpu_gfa import call_text as ug_text
    return ug_text(ya, yb.lib().yakamd_bubbles, h, 1, out, stats=stats)


# ---- what does not fit ----
def test_damaged_inputs(ya, libs, tabs, monkeypatch):
    """each returns -1 (NULL at the open) with its message and the number of misfits in it; none reads or writes outside: the check stands in front
    of the use, as the model has shown on the CPU.  The next call on the same handle works"""
    yw, yg, yb, yp, yl = libs
    AL = yl.lib()
    err = AL.yakamd_allele_last_error
    tab = tabs("two_k5_p10")
    ug, recs = want_of(tab)
    paths, steps = edge_lists(ug, recs, 9)
    want = A.observe(paths, steps, recs, A.arm_map(len(ug), recs))[0]
    ap, st = as_paths(paths), np.array(steps, np.uint64)
    n_u = len(ug)
    with Opened(libs, tab, path=False) as o:
        damaged = []
        s2 = st.copy(); s2[300] = n_u << 1 | 1; damaged.append((ap, s2, b"1 of the 3073 steps"))                 # a step's unitig outside the walk
        s2 = st.copy(); s2[[5, 700, 3072]] = (1 << 40) + 1; damaged.append((ap, s2, b"3 of the 3073 steps"))
        p2 = ap.copy(); p2["n_step"][3] += 1; damaged.append((p2, st, b"steps do not fit"))                      # the next path does not follow it
        p2 = ap.copy(); p2["n_step"][-1] += 1; damaged.append((p2, st, b"steps do not fit"))                     # the last path leaves the steps
        p2 = ap.copy(); p2["step_off"][10] = 1 << 50; damaged.append((p2, st, b"steps do not fit"))
        p2 = ap.copy(); p2["step_off"] = p2["step_off"][::-1].copy(); damaged.append((p2, st, b"steps do not fit"))   # no order at all
        for p2, s2, what in damaged:
            for cap in (None, len(want)):
                rc, n_out, raw = device_obs(ya, o.al, p2, s2, cap, give=cap is not None)
                assert rc == -1 and what in err() and n_out == [0, 0] and raw == b"\xa5" * len(raw), (what, err())
        assert sup_rows(o.al.support()) == [(0, 0, 0, 0)] * len(recs)
        obs, _, _ = o.al.observe(ap, st)
        assert rows(obs) == want
    # the bubbles of one walk with the unitigs of another: at min_cnt 2 the arm seen once is gone, and with it a unitig that the records name
    tab = tabs("closing_k5_p10")
    assert len(want_of(tab, 1)[1]) == 1 and len(want_of(tab, 2)[0]) == 1
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 5) as g, yb.Bubbles(w, g, 5) as b, yw.Walk(tab.t, 2) as w2:
        assert AL.yakamd_allele_open(w2.w, b.b) is None and b"1 arms of the 1 bubbles name none of the 1 unitigs" in err()
        monkeypatch.setenv("YAKAMD_ALLELE_DAMAGE", "dup")
        assert AL.yakamd_allele_open(w.w, b.b) is None and b"1 arms of the 1 bubbles name a unitig that another arm holds" in err()
        monkeypatch.delenv("YAKAMD_ALLELE_DAMAGE")
        with yl.Alleles(w, b) as al:
            assert al.stats()["n_arm"] == 2


def test_refusals(ya, libs, tabs, synth, tmp_path):
    yw, yg, yb, yp, yl = libs
    AL = yl.lib()
    err = AL.yakamd_allele_last_error
    out, fa = str(tmp_path / "o.txt"), str(tmp_path / "s.fa")
    open(fa, "wb").write(b">r\nTTCAGGTCTCATG\n")
    tab = tabs("bubble_k5_p10")
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 5) as g, yb.Bubbles(w, g, 5) as b:
        assert AL.yakamd_allele_open(None, b.b) is None and b"no walk" in err()
        assert AL.yakamd_allele_open(w.w, None) is None and b"no bubbles" in err()
        with yl.Alleles(w, b) as al:
            st = yl.AlstatT()
            assert AL.yakamd_allele_stats(al.al, None) == -1 and AL.yakamd_allele_stats(None, C.byref(st)) == -1
            d = ya.lib().yakamd_dev_alloc(4096)
            try:
                n_out = (C.c_int64 * 2)()
                call = lambda *a: AL.yakamd_allele_obs_dev(al.al, *a)
                assert call(d + 8, 1, d + 1024, 3, d + 2048, 3, n_out) == -1 and b"aligned" in err()
                assert call(d, 1, d + 1028, 3, d + 2048, 3, n_out) == -1 and b"aligned" in err()
                assert call(d, 1, d + 1024, 3, d + 2056, 3, n_out) == -1 and b"aligned" in err()
                assert call(d, -1, d + 1024, 3, None, 0, n_out) == -1 and call(d, 1, d + 1024, -3, None, 0, n_out) == -1
                assert call(None, 1, d + 1024, 3, None, 0, n_out) == -1 and call(d, 1, None, 3, None, 0, n_out) == -1 and b"without" in err()
                assert call(d, 0, d + 1024, 3, None, 0, n_out) == -1 and call(d, 4, d + 1024, 3, None, 0, n_out) == -1 and b"a path has a step or more" in err()
                assert AL.yakamd_allele_obs_dev(al.al, d, 1, d + 1024, 3, None, 0, None) == -1 and b"two numbers" in err()
            finally:
                ya.lib().yakamd_dev_free(d)
    o = yl.AloptT()
    AL.yakamd_alopt_init(C.byref(o))
    for h, field, value, fn, what in ((None, "min_cnt", 1, fa, b"not an engine table"), (tab.t.h, "min_cnt", 0, fa, b"min_cnt 0"), (tab.t.h, "min_cnt", 1024, fa, b"min_cnt 1024"),
                                      (tab.t.h, "min_sup", 0, fa, b"min_sup 0"), (tab.t.h, "min_frag", 0, fa, b"min_frag 0"), (tab.t.h, "chunk_size", 0, fa, b"chunk_size 0"),
                                      (tab.t.h, "min_cnt", 1, fa + ".none", b"cannot read")):
        AL.yakamd_alopt_init(C.byref(o))
        setattr(o, field, value)
        assert AL.yakamd_alleles(C.byref(o), h, fn.encode(), out.encode()) == -1 and what in err(), (what, err())
        assert not os.path.exists(out), "a refused call created its output"
    AL.yakamd_alopt_init(C.byref(o))
    for k, mark, what in ((30, 0, b"even"), (31, 1, b"homopolymer-compressed")):
        t = ya.Table(k, 10, 4, 0)
        try:
            if mark:
                assert ya.lib().yakamd_ch_set_hpc(t.h, 1) == 0
            t.count_pass_host(1, synth(300, 150, 2500, s=5))
            assert AL.yakamd_alleles(C.byref(o), t.h, fa.encode(), out.encode()) == -1 and what in err() and not os.path.exists(out)
        finally:
            t.close()


def test_every_kernel_is_launched(ya, libs, tabs):
    """the six instantiations of the library's tally and no other launch: the open launches the index once, a counting call the count and the three
    kernels of the scan, a writing call those and the emit; nothing of the libraries below is launched by either"""
    yw, yg, yb, yp, yl = libs
    assert set(yl.tally()) == set(KERNELS)
    tab = tabs("two_k5_p10")
    ug, recs = want_of(tab)
    paths, steps = edge_lists(ug, recs, 1)
    ap, st = as_paths(paths), np.array(steps, np.uint64)
    yl.lib().yakamd_allele_tally_reset()
    zero = dict.fromkeys(KERNELS, 0)
    below = lambda: (yw.tally(), yg.tally(), yb.tally(), yp.tally())
    with yw.Walk(tab.t, 1) as w, yg.Gfa(w, 5) as g, yb.Bubbles(w, g, 5) as b:
        before = below()
        with yl.Alleles(w, b) as al:
            assert yl.tally() == dict(zero, k_al_index=1)
            al.observe(ap, st, count_only=True)
            scan = {"k_al_find<COUNT>": 1, "k_al_tile_sum": 1, "k_al_tile_scan": 1, "k_al_scan_apply": 1}
            assert yl.tally() == dict(zero, k_al_index=1, **scan)
            al.observe(ap, st)                                   # a counting call, then a writing one
            assert yl.tally() == dict({k: 3 for k in scan}, **{"k_al_index": 1, "k_al_find<EMIT>": 1})
        assert below() == before
