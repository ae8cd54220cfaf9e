"""The phasing of the bubbles' alleles on the device (the kernels of yak_amd/phase/phase.hip behind yakamd_phase_votes_dev, _pairs_dev, _solve_dev,
_nodes_dev, _edges_dev, _blocks_dev, yakamd_phase, the CLI's `bubbles -r -p` and yak_amd.phase) against the restatement of tests/phase_util.py (held
to a second one, to hand-derived cases and to the sequential model of the kernels by tests/test_phase.py and tests/test_phase_model.py): the nodes and
the blocks element by element, the pairs and the edges as sorted lists, the texts byte for byte.  The shapes are the smallest that can go wrong: a full
record as the last of a workgroup's 256 and as the first of the next, and of the third tile of the scan; fragments across those edges, a fragment that
holds whole workgroups, partial records between two full ones across each edge; more tiles than the scan kernel has threads; 100 000 votes on one
pair; a table that grows feed by feed; feeds that add up, a reset; 4 KiB behind every output; long hook chains, mutual choices, a star, a complete
graph, disjoint pairs; no record and no bubble; damaged inputs, each caught by a bound check that the model has exercised on the CPU; the refusals;
a launch of every kernel."""
import ctypes as C
import gzip
import math
import os
import random
import subprocess

import numpy as np
import pytest

import allele_util as A
import bubble_util as B
import graph_util as U
import path_util as P
import phase_util as PH
from test_allele import TWO
from test_bubble import CIRCLE, HAND
from test_gpu_bubble import many_snps
from test_gpu_graph import CLI, Tab, restated_file
from test_phase import DIPLOID_SEEDS, HAND_TABLES, HET, HOM, KERNELS

pytestmark = pytest.mark.gpu
T = 600
PAD = 4096
WG, TILE = 256, 1024                           # the records of a workgroup of k_ph_full, and of a tile of the scan
NONE = PH.NONE


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the phasing has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def libs(ya):
    import yak_amd.allele
    import yak_amd.bubble
    import yak_amd.gfa
    import yak_amd.path
    import yak_amd.phase
    import yak_amd.walk
    yak_amd.phase.lib()
    return yak_amd.walk, yak_amd.gfa, yak_amd.bubble, yak_amd.path, yak_amd.allele, yak_amd.phase


def diploid_image(seed):
    a, b, pos, behind = PH.diploid(random.Random(seed))
    return U.image([a.encode(), b.encode()])


SHAPES = {
    "circle_k5_p10": lambda: U.image([s.encode() for s in HAND["circle"][1]]), "two_k5_p10": lambda: U.image([s.encode() for s in TWO]),
    "tip_k5_p10": lambda: U.image([s.encode() for s in HAND["tip"][1]]), "manysnps_k15_p10": lambda: many_snps(15, 6000, 15),
}
SHAPES.update({"diploid%d_k15_p10" % seed: (lambda seed=seed: diploid_image(seed)) for seed in DIPLOID_SEEDS})      # the three planted diploids of tests/test_phase.py


@pytest.fixture(scope="module")
def tabs(ya, tmp_path_factory):
    d = tmp_path_factory.mktemp("phase")
    made = {}

    def get(name):
        if name not in made:
            _, k, pre = name.split("_")
            tab = Tab(ya, d, name, SHAPES[name](), int(k[1:]), int(pre[1:]))
            recs, st, ug = tab.restated(1)
            tab.ph_want = (ug, B.by_strings(tab.k, ug)[0])         # (unitigs, bubble records) of the dump, computed once
            made[name] = tab
        return made[name]
    yield get
    for t in made.values():
        t.t.close()


def as_obs(obs):
    from yak_amd.allele import OBS_DTYPE
    return np.array([tuple(o[:4]) for o in obs], OBS_DTYPE) if len(obs) else np.zeros(0, OBS_DTYPE)


def as_sup(sup):
    from yak_amd.allele import SUP_DTYPE
    out = np.zeros(len(sup), SUP_DTYPE)
    for i, s in enumerate(sup):
        out[i] = ((s[0], s[1]), (s[2], s[3]))
    return out


def pair_rows(ph):
    return sorted((int(p["i"]), int(p["j"]), int(p["cis"]), int(p["trans"])) for p in ph.pairs(PAD))


def want_pairs(votes):
    return sorted((i, j, c, t) for (i, j), (c, t) in votes.items())


def solved_equals(ph, n_bubble, sup, votes, min_sup=2, min_link=2):
    """a solve of the device against Kruskal's on the same votes: the nodes and the blocks one by one, the edges as a sorted list, the tallies, and
    the rounds within their bound; returns the device's tallies"""
    st = ph.solve(as_sup(sup), min_sup, min_link)
    res = PH.kruskal(n_bubble, sup, votes, min_sup, min_link)
    assert pair_rows(ph) == want_pairs(votes)
    nodes = ph.nodes(PAD)
    assert [(int(n["block"]), int(n["flags"])) for n in nodes] == [(NONE, 0) if n is None else n for n in res["nodes"]]
    kind = dict(forest=PH.FOREST, conc=0, disc=PH.DISC)
    assert sorted((int(e["i"]), int(e["j"]), int(e["w"]), int(e["flags"])) for e in ph.edges(PAD)) == sorted((i, j, e[0], e[1] | kind[e[2]]) for (i, j), e in res["edges"].items())
    assert [tuple(int(v) for v in b) for b in ph.blocks(PAD)] == res["blocks"]
    want = res["stats"]
    assert {key: st[key] for key in ("n_het", "n_edge", "n_forest", "n_block", "n_single")} == {key: want[key] for key in ("n_het", "n_edge", "n_forest", "n_block", "n_single")}
    assert st["n_bubble"] == n_bubble and st["n_pair"] == len(votes) and st["capacity"] >= 2 * len(votes)
    assert st["n_round"] <= (math.ceil(math.log2(st["n_het"])) + 1 if st["n_edge"] else 0), st
    return st


def fed(yph, n_bubble, chunks_obs):
    """a Phase with the records of the chunks fed, each feed held to the restatement's numbers"""
    ph = yph.Phase(n_bubble)
    for obs in chunks_obs:
        v, n_full, n_vote = PH.votes_flat([obs])
        assert ph.votes(as_obs(obs)) == (n_full, n_vote)
    return ph


# ---- the hand cases and the planted diploid through the device calls ----
def test_hand_cases(libs):
    yph = libs[5]
    rng = random.Random(1)
    for n_bubble, votes, not_het in HAND_TABLES:
        sup = [HOM if b in not_het else HET for b in range(n_bubble)]
        obs = PH.obs_of_votes(votes, rng)
        half = next((x for x in range(len(obs) // 2, len(obs)) if obs[x][0] != obs[x - 1][0]), len(obs))
        first = obs[half][0] if half < len(obs) else 0
        for chunks in ([obs], [obs[:half], [(o[0] - first,) + o[1:] for o in obs[half:]]]):
            with fed(yph, n_bubble, chunks) as ph:
                for m, e in ((2, 2), (1, 1), (2, 3)):              # other minima on the same votes
                    solved_equals(ph, n_bubble, sup, votes, m, e)


class Opened:
    """the arm map and the index of a table; the walk, the links and the bubbles closed once the two stand"""

    def __init__(self, libs, tab):
        yw, yg, yb, yp, yl, yph = libs
        with yw.Walk(tab.t, 1) as w, yg.Gfa(w, tab.k) as g, yb.Bubbles(w, g, tab.k) as b:
            self.al = yl.Alleles(w, b)
            self.px = yp.Path(w, tab.k)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.al.close()
        self.px.close()


def through_the_calls(libs, tab, reads, min_sup=2, min_link=2, chunk_size=1 << 28):
    """reads through the index, the chain, the observations, the votes and the solve of the device, against whole() on the dump"""
    yph = libs[5]
    ug, recs = tab.ph_want
    w = PH.whole(tab.k, ug, recs, reads, min_sup, min_link, chunk_size)
    with Opened(libs, tab) as o, yph.Phase(len(recs)) as ph:
        for part, d in zip(A.chunks(reads, chunk_size), w["per"]):
            img, off, lens = P.image([reads[i] for i in part])
            paths, steps, _ = o.px.chain(img, off, lens)
            obs, n_obs, n_full = o.al.observe(paths, steps)
            assert [tuple(int(v) for v in r) for r in obs] == d["obs"]
            got = ph.votes(obs)
            assert got == PH.votes_flat([d["obs"]])[1:]
        sup = o.al.support()
        assert [(int(s["full"][0]), int(s["full"][1]), int(s["part"][0]), int(s["part"][1])) for s in sup] == w["sup"]
        st = solved_equals(ph, len(recs), w["sup"], w["votes"], min_sup, min_link)
        print("phase", st, "ms", yph.ms())
    return w


def diploid_reads(seed):
    rng = random.Random(seed)
    a, b, pos, behind = PH.diploid(rng)
    return PH.diploid_reads(rng, (a, b), 240)


def test_reads_through_real_bubbles(libs, tabs):
    reads = [r.encode() for r in (TWO[0], TWO[1], U.rc_str(TWO[0][:14] + TWO[1][14:]), TWO[0][:15], TWO[1][12:], TWO[0], TWO[1])]
    for chunk_size in (1 << 28, 40):
        w = through_the_calls(libs, tabs("two_k5_p10"), reads, chunk_size=chunk_size)
        assert sorted(w["votes"].values()) == [[4, 1]] and w["res"]["stats"]["n_block"] == 1
    read = CIRCLE * 2 + CIRCLE[:8]
    w = through_the_calls(libs, tabs("circle_k5_p10"), [read.encode(), U.rc_str(read).encode()], min_sup=1)
    assert (w["n_full"], w["n_vote"]) == (4, 0)                    # twice round the circle: no vote


def test_planted_diploids(libs, tabs):
    for seed in DIPLOID_SEEDS:
        for chunk_size in (1 << 28, 5000):
            w = through_the_calls(libs, tabs("diploid%d_k15_p10" % seed), diploid_reads(seed), chunk_size=chunk_size)
            st = w["res"]["stats"]
            assert (st["n_block"], st["n_single"], st["n_disc"]) == (2, 0, 0) and st["n_het"] >= 40 and w["n_vote"] > 300, seed


# ---- record lists of the test's own making ----
def edge_records(seed, partial_at_edges):
    """records with a full one at 255, 256, 3071 and 3072 (the last of a workgroup and the first of the next; of the third tile of the scan) -- or, with
    partial_at_edges, partial ones there between two full ones at 254 and 257, 3070 and 3073 --, a fragment that straddles each of the two edges, one
    that holds two whole workgroups (500 .. 1030, across the first tile's edge as well), and short random ones; 40 bubbles"""
    rng = random.Random(seed)
    n = 3 * TILE + 40
    cuts = {0, 250, 262, 500, 1031, 3066, 3080}                    # where the planned fragments begin and end
    at = 0
    while at < n:
        at += rng.choice((1, 2, 3, 3, 5, 9))
        if not any(lo < at < hi for lo, hi in ((250, 262), (500, 1031), (3066, 3080))):
            cuts.add(at)
    obs, seq = [], -1
    for t in range(n):
        if t in cuts:
            seq += 1
        full = rng.random() < 0.7
        if t in (255, 256, 3071, 3072):
            full = not partial_at_edges
        if t in (254, 257, 3070, 3073):
            full = True
        obs.append((seq, rng.randrange(40), (PH.FULL if full else 0) | rng.randrange(2) | 4 * rng.randrange(2), rng.randrange(7)))
    return obs


def test_records_at_the_edges_of_workgroups_and_tiles(libs):
    yph = libs[5]
    for seed, partial in ((1, False), (2, True), (3, False)):
        obs = edge_records(seed, partial)
        assert all(bool(obs[t][2] & PH.FULL) != partial for t in (255, 256, 3071, 3072)) and obs[255][0] == obs[256][0] and obs[3071][0] == obs[3072][0]
        assert obs[500][0] == obs[1030][0] and obs[254][0] == obs[257][0] and obs[3070][0] == obs[3073][0]
        votes, n_full, n_vote = PH.votes_flat([obs])
        assert n_vote > 1000 and len(votes) > 400
        with fed(yph, 40, [obs]) as ph:
            assert pair_rows(ph) == want_pairs(votes)
            solved_equals(ph, 40, [HET] * 39 + [HOM], votes, 2, 1)


def test_more_tiles_than_the_tile_scan_has_threads(libs):
    """257 tiles and some: every thread of the one workgroup that scans the tile sums has a tile, the first two"""
    yph = libs[5]
    rng = np.random.default_rng(7)
    n = 257 * TILE + 300
    from yak_amd.allele import OBS_DTYPE
    obs = np.zeros(n, OBS_DTYPE)
    obs["seq"] = np.arange(n) // 3                               # fragments of up to three entries
    obs["bubble"] = rng.integers(0, 50, n)
    obs["flags"] = rng.integers(0, 8, n)
    rows = list(zip(obs["seq"].tolist(), obs["bubble"].tolist(), obs["flags"].tolist(), obs["path"].tolist()))
    votes, n_full, n_vote = PH.votes_flat([rows])
    with yph.Phase(50) as ph:
        assert ph.votes(obs) == (n_full, n_vote) and n_full > 100000
        assert pair_rows(ph) == want_pairs(votes) and len(votes) == 50 * 49 // 2


def test_a_hundred_thousand_votes_on_one_pair(libs):
    yph = libs[5]
    from yak_amd.allele import OBS_DTYPE
    n = 100001
    obs = np.zeros(n, OBS_DTYPE)                                 # one fragment that goes to and fro between bubbles 0 and 1
    obs["bubble"] = np.arange(n) & 1
    obs["flags"] = PH.FULL | (np.arange(n) % 3 == 0)
    a = obs["flags"] & 1
    trans = int(np.count_nonzero(a[1:] != a[:-1]))
    with yph.Phase(2) as ph:
        assert ph.votes(obs) == (n, n - 1)
        assert pair_rows(ph) == [(0, 1, n - 1 - trans, trans)] and 0 < trans < n - 1
        assert ph.stats()["n_pair"] == 1


def test_the_table_grows_feed_by_feed(libs):
    """a complete graph on 40 bubbles fed in six feeds of 3, 10, 30, 90, 250 and 397 new pairs: the table grows from 16 slots three times or more, and
    after every feed the pairs are those fed so far; feeds add up; a reset empties the table and keeps its capacity"""
    yph = libs[5]
    rng = random.Random(4)
    n = 40
    all_pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    rng.shuffle(all_pairs)
    votes, grows = {}, []
    with yph.Phase(n) as ph:
        assert ph.stats()["capacity"] == 16 and ph.stats()["n_grow"] == 0
        for lo, hi in ((0, 3), (3, 13), (13, 43), (43, 133), (133, 383), (383, 780)):
            mine = {p: [rng.randint(0, 1), 1] for p in all_pairs[lo:hi] + all_pairs[:3]}      # three pairs are voted in every feed
            obs = PH.obs_of_votes(mine, rng)
            for p, v in mine.items():
                votes[p] = [x + y for x, y in zip(votes.get(p, [0, 0]), v)]
            assert ph.votes(as_obs(obs)) == PH.votes_flat([obs])[1:]
            st = ph.stats()
            grows.append(st["n_grow"])
            assert pair_rows(ph) == want_pairs(votes) and st["n_pair"] == len(votes) and st["capacity"] >= 2 * len(votes)
        assert grows == sorted(grows) and grows[-1] >= 3 and len(votes) == 780
        solved_equals(ph, n, [HET] * n, votes, 2, 1)
        cap = ph.stats()["capacity"]
        ph.reset()
        assert ph.stats()["n_pair"] == 0 and ph.stats()["capacity"] == cap and len(ph.pairs()) == 0
        with pytest.raises(RuntimeError, match="no solve since"):
            ph.nodes()
        few = {(0, 1): [2, 0], (1, 2): [0, 3]}
        obs = PH.obs_of_votes(few, rng)
        for _ in range(3):
            ph.votes(as_obs(obs))
        solved_equals(ph, n, [HET] * n, {p: [3 * v[0], 3 * v[1]] for p, v in few.items()})


# ---- the solves ----
def fragments_of(weights):
    """records whose votes are {(i, j): (w, trans)}: one fragment per pair that goes to and fro between its two bubbles, w + 1 entries"""
    from yak_amd.allele import OBS_DTYPE
    lens = np.array([w + 1 for (w, t) in weights.values()], np.int64)
    n = int(lens.sum())
    start = np.cumsum(lens) - lens
    seq = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(n) - np.repeat(start, lens)
    i = np.repeat(np.array([p[0] for p in weights], np.int64), lens)
    j = np.repeat(np.array([p[1] for p in weights], np.int64), lens)
    trans = np.repeat(np.array([t for (w, t) in weights.values()], np.int64), lens)
    obs = np.zeros(n, OBS_DTYPE)
    obs["seq"], obs["bubble"], obs["flags"] = seq, np.where(within & 1, j, i), PH.FULL | (within & 1 & trans)
    return obs


def solve_case(yph, n_bubble, weights, min_link=1):
    votes = {p: ([0, w] if t else [w, 0]) for p, (w, t) in weights.items()}
    with yph.Phase(n_bubble) as ph:
        assert ph.votes(fragments_of(weights)) == (sum(w + 1 for w, t in weights.values()), sum(w for w, t in weights.values()))
        st = solved_equals(ph, n_bubble, [HET] * n_bubble, votes, 2, min_link)
        print("solve", st, "ms", yph.ms())
        return st


def test_a_chain_with_rising_weights(libs):
    """5 000 bubbles, edge (i, i + 1) of weight i + 1: every bubble but the last chooses the edge to its right, the longest chain of hooks"""
    st = solve_case(libs[5], 5000, {(i, i + 1): (i + 1, i % 3 == 0) for i in range(4999)})
    assert (st["n_forest"], st["n_block"]) == (4999, 1)


def test_a_chain_with_equal_weights(libs):
    """the same chain, every weight 2: mutual choices, and ties decided by (i, j)"""
    st = solve_case(libs[5], 5000, {(i, i + 1): (2, i % 3 == 0) for i in range(4999)})
    assert (st["n_forest"], st["n_block"]) == (4999, 1)


def test_a_star_a_complete_graph_and_disjoint_pairs(libs):
    rng = random.Random(6)
    st = solve_case(libs[5], 400, {(0, j): (rng.randint(1, 9), rng.randrange(2)) for j in range(1, 400)})
    assert (st["n_forest"], st["n_block"], st["n_round"]) == (399, 1, 2)
    st = solve_case(libs[5], 64, {(i, j): (rng.randint(1, 6), rng.randrange(2)) for i in range(64) for j in range(i + 1, 64)}, min_link=2)
    assert st["n_block"] == 1 and st["n_forest"] == 63 and st["n_edge"] > 1500
    st = solve_case(libs[5], 2000, {(2 * i, 2 * i + 1): (rng.randint(1, 3), rng.randrange(2)) for i in range(1000)})
    assert (st["n_forest"], st["n_block"], st["n_round"]) == (1000, 1000, 2)


# ---- the command ----
def call_text(yph, h, fn, out, **kw):
    o = yph.PhoptT()
    yph.lib().yakamd_phopt_init(C.byref(o))
    for f, v in kw.items():
        setattr(o, f, v)
    if os.path.exists(out):
        os.remove(out)
    assert yph.lib().yakamd_phase(C.byref(o), h, fn.encode(), out.encode()) == 0, yph._err()
    return open(out, "rb").read()


def text_of(k, recs, w, **kw):
    return PH.text(k, 1, kw.get("min_sup", 2), kw.get("min_link", 2), kw.get("edges", 0), kw.get("stats_only", 0), recs, w["sup"], w["head"], w["votes"], w["n_vote"], w["res"])


def test_command_texts(ya, libs, tabs, tmp_path):
    """yakamd_phase on the resident table in three chunk sizes from FASTA, FASTQ and gzip, with -s, -e, -m and -w; the CLI and yak_amd.phase on its
    file (the listing order, and with it the numbering, is the restored table's); every A line is that of `bubbles -r`"""
    yl, yph = libs[4], libs[5]
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
    ug, recs = tab.ph_want
    solved = {}

    def want(ug, recs, key, **kw):
        m, e = kw.get("min_sup", 2), kw.get("min_link", 2)
        if (key, m, e) not in solved:
            solved[(key, m, e)] = PH.whole(15, ug, recs, reads, m, e)
        return text_of(15, recs, solved[(key, m, e)], **kw)
    text = lambda **kw: want(ug, recs, "resident", **kw)
    base = solved.setdefault(("resident", 2, 2), PH.whole(15, ug, recs, reads, 2, 2))
    st = base["res"]["stats"]
    assert st["n_block"] >= 3 and st["max_block"] >= 5 and st["n_edge"] > 50 and text(min_sup=1) != text() != text(min_link=4) and text(edges=1).count(b"\nE\t") == st["n_edge"]
    for fn in (fa, fq, fa + ".gz"):
        for chunk in (1, 3000, 1 << 28):
            assert call_text(yph, tab.t.h, fn, out, chunk_size=chunk, edges=1) == text(edges=1), (fn, chunk)
            assert call_text(yph, tab.t.h, fn, out, chunk_size=chunk) == text()
            assert call_text(yph, tab.t.h, fn, out, chunk_size=chunk, stats_only=1, edges=1) == text(stats_only=1)
    for kw in (dict(min_sup=1), dict(min_sup=3, edges=1), dict(min_link=4, edges=1), dict(min_link=1, min_sup=1, edges=1), dict(stats_only=1)):
        assert call_text(yph, tab.t.h, fa, out, **kw) == text(**kw), kw
    assert call_text(yph, tab.t.h, fa, out, min_cnt=2).startswith(b"#phase\tk=15\tmin_cnt=2\tmin_sup=2\tmin_link=2\nT\t151\t")      # nothing forks at 2
    print("command ms", yph.ms())
    # the file's table
    k, ugf, recsf = on_the_file(ya, tab, tmp_path)
    text = lambda **kw: want(ugf, recsf, "file", **kw)
    run = lambda a: subprocess.run([CLI, "bubbles"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=T).stdout
    assert run(["-r", fa, "-p", tab.fn]) == text() == yph.phase(tab.fn, fa) == yph.phase(tab.fn, fq, chunk_size=1)
    assert run(["-r", fq, "-p", "-e", tab.fn]) == text(edges=1) == yph.phase(tab.fn, fa + ".gz", edges=True)
    assert run(["-p", "-e", "-w4", "-m", "3", "-r", fa + ".gz", tab.fn]) == text(edges=1, min_link=4, min_sup=3) == yph.phase(tab.fn, fa, edges=True, min_link=4, min_sup=3)
    assert run(["-s", "-p", "-r", fa, tab.fn]) == text(stats_only=1) == yph.phase(tab.fn, fa, stats_only=True)
    assert run(["-r", fa, "-p", "-o", out + "2", tab.fn]) == b"" and open(out + "2", "rb").read() == text()
    os.remove(out + "2")
    # every A line is that of `bubbles -r`, and `bubbles -r` is what it was
    plain = run(["-r", fa, tab.fn])
    assert plain == yl.alleles(tab.fn, fa) and [ln for ln in plain.splitlines() if ln[:1] == b"A"] == [ln for ln in text().splitlines() if ln[:1] == b"A"]
    for a in (["-r", fa + ".none", "-p"], ["-r", fa, "-p", "-w", "0"], ["-r", fa, "-p", "-m", "0"], ["-p"], ["-r", fa, "-e"], ["-r", fa, "-p", "-f"]):
        q = subprocess.run([CLI, "bubbles", "-o", out + "2"] + a + [tab.fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
        assert q.returncode != 0 and q.stdout == b"" and q.stderr and not os.path.exists(out + "2"), a


def on_the_file(ya, tab, tmp_path):
    """(k, unitigs, bubble records) of the table restored from tab's file: the CLI and yak_amd.phase number the unitigs as that table lists them"""
    back = ya.Table(ptr=ya.lib().yak_ch_restore(tab.fn.encode()))
    try:
        f = str(tmp_path / "restored.yak")
        open(f, "wb").write(back.dump_bytes())
    finally:
        back.close()
    k, _, _, ugf = restated_file(f, 1)
    return k, ugf, B.by_strings(k, ugf)[0]


def test_the_command_on_the_hand_cases(ya, libs, tabs, tmp_path):
    """the two hand cases that have reads -- the vote tables of HAND_TABLES have none, they go through the device calls in test_hand_cases --
    through yakamd_phase, the CLI and yak_amd.phase: the reads through the two SNPs of TWO, and twice round the circle, held to the restatement
    on the very table and to the H, K, E and T lines that tests/test_phase.py writes out (the A lines name unitigs, whose numbers are the table's)"""
    yph = libs[5]
    fa, out = str(tmp_path / "h.fa"), str(tmp_path / "o.txt")
    read = CIRCLE * 2 + CIRCLE[:8]
    cases = (("two_k5_p10", [TWO[0], TWO[1], U.rc_str(TWO[0][:14] + TWO[1][14:]), TWO[0][:15], TWO[1][12:], TWO[0], TWO[1]], 2,
              ["#phase\tk=5\tmin_cnt=1\tmin_sup=2\tmin_link=2", "H\t0\t0\t0", "H\t1\t0\t0", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t4\t1\tforest",
               "T\t7\t183\t7\t37\t12\t12\t5\t1\t2\t2\t1\t1\t0\t1\t0\t2"]),
             ("circle_k5_p10", [read, U.rc_str(read)], 1, ["#phase\tk=5\tmin_cnt=1\tmin_sup=1\tmin_link=2", "T\t2\t68\t2\t12\t6\t4\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0"]))
    for name, reads, m, written in cases:
        tab = tabs(name)
        reads = [r.encode() for r in reads]
        open(fa, "wb").write(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
        ug, recs = tab.ph_want
        w = PH.whole(5, ug, recs, reads, min_sup=m)
        for chunk in (1 << 28, 40, 1):
            got = call_text(yph, tab.t.h, fa, out, chunk_size=chunk, edges=1, min_sup=m)
            assert got == text_of(5, recs, w, edges=1, min_sup=m), (name, chunk)
            assert [ln for ln in got.decode().splitlines() if ln[0] != "A"] == written, (name, chunk)
        assert call_text(yph, tab.t.h, fa, out, stats_only=1, min_sup=m).decode().splitlines() == [written[0], written[-1]]
        k, ugf, recsf = on_the_file(ya, tab, tmp_path)
        wf = PH.whole(5, ugf, recsf, reads, min_sup=m)
        cli = subprocess.run([CLI, "bubbles", "-r", fa, "-p", "-e", "-m", str(m), tab.fn], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=T).stdout
        assert cli == text_of(5, recsf, wf, edges=1, min_sup=m) == yph.phase(tab.fn, fa, edges=True, min_sup=m, chunk_size=40), name
        assert [ln for ln in cli.decode().splitlines() if ln[0] != "A"] == written, name


def test_the_command_on_the_planted_diploids_and_without_a_bubble(ya, libs, tabs, tmp_path):
    yph = libs[5]
    fa, out = str(tmp_path / "d.fa"), str(tmp_path / "o.txt")
    for seed in DIPLOID_SEEDS:
        tab = tabs("diploid%d_k15_p10" % seed)
        reads = diploid_reads(seed)
        open(fa, "wb").write(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
        ug, recs = tab.ph_want
        w = PH.whole(15, ug, recs, reads)
        for chunk in (1 << 28, 7000):
            got = call_text(yph, tab.t.h, fa, out, chunk_size=chunk, edges=1)
            assert got == text_of(15, recs, w, edges=1), (seed, chunk)
        assert got.count(b"\nK\t") == 2 and got.count(b"\tdisc\n") == 0
        k, ugf, recsf = on_the_file(ya, tab, tmp_path)
        want = text_of(15, recsf, PH.whole(15, ugf, recsf, reads), edges=1)
        cli = subprocess.run([CLI, "bubbles", "-r", fa, "-p", "-e", tab.fn], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=T).stdout
        assert cli == want == yph.phase(tab.fn, fa, edges=True, chunk_size=7000), seed
    tab = tabs("tip_k5_p10")                                         # a graph without a bubble: the header and a T line
    open(fa, "wb").write(b">a\nTTCAGGACTCATG\n>b\nCAGGAGG\n")
    assert call_text(yph, tab.t.h, fa, out) == b"#phase\tk=5\tmin_cnt=1\tmin_sup=2\tmin_link=2\nT\t2\t20\t2\t4\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n"


# ---- the launches ----
def test_no_record_and_no_bubble_launch_nothing(libs):
    yph = libs[5]
    with yph.Phase(0) as ph0, yph.Phase(3) as ph:
        yph.lib().yakamd_phase_tally_reset()
        assert ph.votes(as_obs([])) == (0, 0) and ph0.votes(as_obs([])) == (0, 0)
        st = ph0.solve(as_sup([]))
        assert (st["n_bubble"], st["n_het"], st["n_round"]) == (0, 0, 0) and len(ph0.nodes()) == len(ph0.edges()) == len(ph0.blocks()) == len(ph0.pairs()) == 0
        assert not any(yph.tally().values())
        with pytest.raises(RuntimeError, match="1 of the 1 records do not fit"):
            ph0.votes(as_obs([(0, 0, PH.FULL, 0)]))                  # no bubble: every record names none


def test_the_launches_per_call_and_every_kernel(libs):
    """an open clears the table; a feed counts, scans, writes the entries and votes, and before that grows the table if it must; a getter of the
    pairs counts, scans and writes; a solve of r rounds launches the best w r times and the four kernels behind it r - 1 times"""
    yph = libs[5]
    assert set(yph.tally()) == set(KERNELS)
    zero = dict.fromkeys(KERNELS, 0)
    scan = lambda n: {"k_ph_tile_sum": n, "k_ph_tile_scan": n, "k_ph_scan_apply": n}
    rng = random.Random(3)
    votes = {(i, j): [3, 0] for i in range(8) for j in range(i + 1, 8)}
    yph.lib().yakamd_phase_tally_reset()
    with yph.Phase(8) as ph:
        assert yph.tally() == dict(zero, k_ph_clear=1)
        ph.votes(as_obs(PH.obs_of_votes({(0, 1): [1, 0]}, rng)))     # two entries: the table stays at 16 slots
        feed = {"k_ph_full<COUNT>": 1, "k_ph_full<EMIT>": 1, "k_ph_vote": 1}
        assert yph.tally() == dict(zero, k_ph_clear=1, **feed, **scan(1))
        ph.votes(as_obs(PH.obs_of_votes(votes, rng)))                # 28 pairs: it grows
        assert yph.tally() == dict(zero, k_ph_clear=2, k_ph_rehash=1, **{k: 2 for k in feed}, **scan(2)) and ph.stats()["n_grow"] == 1
        ph.votes(as_obs([(0, 0, PH.FULL, 0), (0, 1, 0, 0)]))         # one full record: counted, and nothing to vote
        assert yph.tally()["k_ph_full<COUNT>"] == 3 and yph.tally()["k_ph_full<EMIT>"] == 2 and yph.tally()["k_ph_vote"] == 2
        yph.lib().yakamd_phase_tally_reset()
        assert len(ph.pairs()) == 28
        assert yph.tally() == dict(zero, **{"k_ph_pairs<COUNT>": 1, "k_ph_pairs<EMIT>": 1}, **scan(1))
        yph.lib().yakamd_phase_tally_reset()
        st = ph.solve(as_sup([HET] * 8), 2, 1)
        r = st["n_round"]
        assert r >= 2 and yph.tally() == dict(zero, k_ph_init=1, k_ph_best_w=r, k_ph_best_key=r - 1, k_ph_hook=r - 1, k_ph_flatten=r - 1, k_ph_rewrite=r - 1, k_ph_name=1,
                                             k_ph_nodes=1, k_ph_classify=1, **{"k_ph_edges<COUNT>": 1, "k_ph_edges<EMIT>": 1, "k_ph_blocks<COUNT>": 1, "k_ph_blocks<EMIT>": 1}, **scan(2))
        yph.lib().yakamd_phase_tally_reset()
        ph.nodes(); ph.edges(); ph.blocks()
        assert not any(yph.tally().values())                       # the results stand since the solve


# ---- what does not fit ----
def test_damaged_inputs_and_refusals(ya, libs, monkeypatch):
    """each returns -1 with its message and the number of misfits in it, adds nothing and writes nothing: the check stands in front of the use, as
    the model has shown on the CPU.  The next call on the same handle works"""
    yph = libs[5]
    L = yph.lib()
    err = L.yakamd_phase_last_error
    rng = random.Random(9)
    votes = {(0, 1): [0, 4], (1, 2): [3, 0], (2, 3): [0, 2]}
    obs = as_obs(PH.obs_of_votes(votes, rng))
    with yph.Phase(4) as ph:
        for get in (ph.nodes, ph.edges, ph.blocks):                  # before a solve
            with pytest.raises(RuntimeError, match="no solve since"):
                get()
        ph.votes(obs)
        bad = obs.copy(); bad["bubble"][[3, 7]] = (4, 1 << 31)
        with pytest.raises(RuntimeError, match="2 of the %d records do not fit" % len(obs)):
            ph.votes(bad)
        bad = obs.copy(); bad["seq"][5] = bad["seq"][-1] + 1
        with pytest.raises(RuntimeError, match="1 of the %d records do not fit" % len(obs)):
            ph.votes(bad)
        assert pair_rows(ph) == want_pairs(votes)                    # nothing was added
        for n_sup in (3, 5):
            with pytest.raises(RuntimeError, match="the support of %d bubbles for 4" % n_sup):
                ph.solve(as_sup([HET] * n_sup))
        for m, e in ((0, 2), (2, 0)):
            with pytest.raises(RuntimeError, match="both are at least 1"):
                ph.solve(as_sup([HET] * 4), m, e)
        with pytest.raises(RuntimeError, match="no solve since"):
            ph.nodes()
        d = ya.lib().yakamd_dev_alloc(2 * PAD)
        try:
            n_out = (C.c_int64 * 2)(7, 7)
            assert L.yakamd_phase_votes_dev(ph.ph, d + 8, 2, n_out) == -1 and b"aligned" in err() and list(n_out) == [0, 0]
            assert L.yakamd_phase_votes_dev(ph.ph, d, -1, n_out) == -1 and L.yakamd_phase_votes_dev(ph.ph, None, 2, n_out) == -1 and b"without their list" in err()
            assert L.yakamd_phase_votes_dev(ph.ph, d, 2, None) == -1 and b"two numbers" in err()
            assert L.yakamd_phase_solve_dev(ph.ph, d + 8, 4, 2, 2) == -1 and b"aligned" in err()
            yph.lib().yakamd_phase_tally_reset()
            assert L.yakamd_phase_pairs_dev(ph.ph, d + 8, 3) == -1 and b"aligned" in err() and L.yakamd_phase_pairs_dev(ph.ph, d, 2) == 3
            assert not any(yph.tally().values())                     # both answered before any launch
        finally:
            ya.lib().yakamd_dev_free(d)
        solved_equals(ph, 4, [HET] * 4, votes)
        assert ph.votes(as_obs([(0, 0, PH.FULL, 0), (0, 1, 0, 0)])) == (1, 0)      # a feed that votes nothing is a feed: the results no longer stand
        with pytest.raises(RuntimeError, match="no solve since"):
            ph.blocks()
        solved_equals(ph, 4, [HET] * 4, votes)
    # the vote limit, lowered by the test switch: a feed that could reach it is refused before any launch
    monkeypatch.setenv("YAKAMD_PHASE_VOTE_LIMIT", "12")
    with yph.Phase(4) as ph:
        monkeypatch.delenv("YAKAMD_PHASE_VOTE_LIMIT")
        few = as_obs(PH.obs_of_votes({(0, 1): [0, 4]}, None))        # eight records: four votes, and up to seven
        assert ph.votes(few) == (8, 4)
        yph.lib().yakamd_phase_tally_reset()
        with pytest.raises(RuntimeError, match="4 votes so far and up to 8 more"):
            ph.votes(as_obs(PH.obs_of_votes({(0, 1): [0, 4], (1, 2): [1, 0]}, None)[:9]))
        assert not any(yph.tally().values()) and pair_rows(ph) == [(0, 1, 0, 4)]
        assert ph.votes(few) == (8, 4) and pair_rows(ph) == [(0, 1, 0, 8)]      # 4 + 7 stays below 12
    o = yph.PhoptT()
    L.yakamd_phopt_init(C.byref(o))
    assert L.yakamd_phase(C.byref(o), None, b"reads.fa", b"out.txt") == -1 and b"not an engine table" in err() and not os.path.exists("out.txt")
