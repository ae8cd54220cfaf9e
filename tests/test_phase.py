"""The phasing of the bubbles' alleles from read support (`yak-amd bubbles -r -p`) without a GPU: the restatements of
tests/phase_util.py -- the votes from the observation records and from the F lines, the solve by Kruskal's algorithm and from the definition -- held
to each other, with all texts, on a few hundred tiny random vote tables, on hand-derived cases whose H, K and E lines are written out here, and on
planted diploid genomes, where the phase of every block must be that of the planted haplotypes and the long gap must part two blocks; the
invariants include/yak_amd_phase.h promises.  Last, libyak_amd_phase.so itself: its exports, its own launch tally, the sizes of its structs, what
it is linked against, and its refusals and the command line's, which need no device.  The tests of the restatement use tests/phase_util.py alone:
they hold the definition to itself and need no library, so they pass where the library is missing; the three tests of the library and of the
command line at the end, tests/test_phase_model.py and tests/test_gpu_phase.py are the ones that fail without the feature."""
import ctypes as C
import os
import random
import re
import subprocess

import allele_util as A
import bubble_util as B
import graph_util as U
import phase_util as PH
from conftest import ROOT
from test_allele import TWO, graph_of, names_of
from test_bubble import CIRCLE, HAND

KERNELS = ["k_ph_full<COUNT>", "k_ph_full<EMIT>", "k_ph_tile_sum", "k_ph_tile_scan", "k_ph_scan_apply", "k_ph_clear", "k_ph_rehash", "k_ph_vote", "k_ph_pairs<COUNT>",
           "k_ph_pairs<EMIT>", "k_ph_edges<COUNT>", "k_ph_edges<EMIT>", "k_ph_init", "k_ph_best_w", "k_ph_best_key", "k_ph_hook", "k_ph_flatten", "k_ph_rewrite", "k_ph_name",
           "k_ph_nodes", "k_ph_classify", "k_ph_blocks<COUNT>", "k_ph_blocks<EMIT>"]
# the seeds of the planted diploids: fixed, and what they must give is asserted in test_planted_diploids below
DIPLOID_SEEDS = (1, 4, 9)
HET, HOM = (2, 2, 0, 0), (2, 0, 0, 0)
# the hand-derived vote tables of the tests below: (bubbles, votes, the bubbles that are not het)
HAND_TABLES = [(2, {(0, 1): [3, 0]}, ()), (2, {(0, 1): [0, 3]}, ()), (2, {(0, 1): [2, 2]}, ()), (2, {(0, 1): [3, 2]}, ()), (2, {(0, 1): [4, 2]}, ()),
               (3, {(0, 1): [5, 0], (1, 2): [5, 0]}, (1,)), (3, {(0, 1): [3, 0], (1, 2): [2, 0], (0, 2): [0, 1]}, ()), (3, {(0, 1): [2, 0], (0, 2): [0, 2], (1, 2): [2, 0]}, ()),
               (4, {(0, 1): [0, 4], (1, 2): [3, 0], (2, 3): [0, 2]}, ()), (5, {(0, 3): [2, 0], (1, 2): [0, 2]}, ()), (3, {}, ())]


def both(n_bubble, sup, votes, min_sup=2, min_link=2):
    """the two solves, which must agree in everything; the result with its lines"""
    res = PH.kruskal(n_bubble, sup, votes, min_sup, min_link)
    assert res == PH.by_definition(n_bubble, sup, votes, min_sup, min_link)
    st = res["stats"]
    assert st["n_forest"] == st["n_het"] - st["n_block"] - st["n_single"] == sum(1 for e in res["edges"].values() if e[2] == "forest")
    assert all(n is None or res["nodes"][n[0]] == (n[0], 0) for n in res["nodes"])            # a block's name has h = 0 and names itself
    return res


def hand(n_bubble, votes, not_het=(), min_sup=2, min_link=2):
    sup = [HOM if b in not_het else HET for b in range(n_bubble)]
    res = both(n_bubble, sup, votes, min_sup, min_link)
    # the votes come back from records of the test's own making, and from the F lines of those records
    obs = PH.obs_of_votes(votes, random.Random(len(votes)))
    got, n_full, n_vote = PH.votes_flat([obs])
    assert got == {p: v for p, v in votes.items() if v != [0, 0]} and n_vote == sum(c + t for c, t in votes.values()) and n_full == 2 * n_vote
    names = ["r%d" % s for s in range(n_vote)]
    assert PH.votes_from_f_lines(A.frag_lines(names, obs, 1)) == (got, n_full, n_vote)
    return [ln.rstrip("\n") for ln in PH.lines_of(res, True)]


def test_two_bubbles_cis_and_trans():
    assert hand(2, {(0, 1): [3, 0]}) == ["H\t0\t0\t0", "H\t1\t0\t0", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t3\t0\tforest"]
    assert hand(2, {(0, 1): [0, 3]}) == ["H\t0\t0\t0", "H\t1\t0\t1", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t0\t3\tforest"]
    assert hand(2, {(0, 1): [1, 4]}) == ["H\t0\t0\t0", "H\t1\t0\t1", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t1\t4\tforest"]


def test_a_tie_is_never_an_edge():
    assert hand(2, {(0, 1): [2, 2]}) == ["H\t0\t0\t0", "H\t1\t1\t0"]
    assert hand(2, {(0, 1): [2, 2]}, min_link=1) == ["H\t0\t0\t0", "H\t1\t1\t0"]


def test_min_link_is_the_first_weight_that_links():
    """w = e - 1 against w = e"""
    assert hand(2, {(0, 1): [3, 2]}) == ["H\t0\t0\t0", "H\t1\t1\t0"]
    assert hand(2, {(0, 1): [4, 2]}) == ["H\t0\t0\t0", "H\t1\t0\t0", "K\t0\t2\t1\t0\t2\t0", "E\t0\t1\t4\t2\tforest"]
    assert hand(2, {(0, 1): [4, 2]}, min_link=3) == ["H\t0\t0\t0", "H\t1\t1\t0"]
    assert hand(2, {(0, 1): [2, 5]}, min_link=3) == ["H\t0\t0\t0", "H\t1\t0\t1", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t2\t5\tforest"]


def test_an_endpoint_that_is_not_het():
    """bubble 1 is hom1: its pairs are no edges, it has no H line, and bubbles 0 and 2 stay alone"""
    assert hand(3, {(0, 1): [5, 0], (1, 2): [5, 0]}, not_het=(1,)) == ["H\t0\t0\t0", "H\t2\t2\t0"]


def test_a_frustrated_triangle():
    """weights 3, 2, 1: the two heavier edges are the forest and say all three are in phase; the edge of weight 1 says trans: discordant"""
    assert hand(3, {(0, 1): [3, 0], (1, 2): [2, 0], (0, 2): [0, 1]}, min_link=1) == [
        "H\t0\t0\t0", "H\t1\t0\t0", "H\t2\t0\t0", "K\t0\t3\t3\t1\t6\t1", "E\t0\t1\t3\t0\tforest", "E\t0\t2\t0\t1\tdisc", "E\t1\t2\t2\t0\tforest"]
    # equal weights: (0, 1) and (0, 2) come first, so bubble 2 is trans to both others, and the cis edge (1, 2) is discordant
    assert hand(3, {(0, 1): [2, 0], (0, 2): [0, 2], (1, 2): [2, 0]}) == [
        "H\t0\t0\t0", "H\t1\t0\t0", "H\t2\t0\t1", "K\t0\t3\t3\t1\t6\t2", "E\t0\t1\t2\t0\tforest", "E\t0\t2\t0\t2\tforest", "E\t1\t2\t2\t0\tdisc"]
    # a triangle that agrees: the third edge is concordant
    assert hand(3, {(0, 1): [2, 0], (0, 2): [0, 2], (1, 2): [0, 2]}) == [
        "H\t0\t0\t0", "H\t1\t0\t0", "H\t2\t0\t1", "K\t0\t3\t3\t0\t6\t0", "E\t0\t1\t2\t0\tforest", "E\t0\t2\t0\t2\tforest", "E\t1\t2\t0\t2\tconc"]


def test_a_chain():
    assert hand(4, {(0, 1): [0, 4], (1, 2): [3, 0], (2, 3): [0, 2]}) == [
        "H\t0\t0\t0", "H\t1\t0\t1", "H\t2\t0\t1", "H\t3\t0\t0", "K\t0\t4\t3\t0\t9\t0", "E\t0\t1\t0\t4\tforest", "E\t1\t2\t3\t0\tforest", "E\t2\t3\t0\t2\tforest"]


def test_two_blocks_and_a_singleton():
    assert hand(5, {(0, 3): [2, 0], (1, 2): [0, 2]}) == [
        "H\t0\t0\t0", "H\t1\t1\t0", "H\t2\t1\t1", "H\t3\t0\t0", "H\t4\t4\t0", "K\t0\t2\t1\t0\t2\t0", "K\t1\t2\t1\t0\t2\t0", "E\t0\t3\t2\t0\tforest", "E\t1\t2\t0\t2\tforest"]


def test_min_sup_and_min_link_changed_on_the_same_votes():
    votes = {(0, 1): [3, 0], (1, 2): [0, 1]}
    sup = [(3, 3, 0, 0), (2, 2, 0, 0), (3, 1, 0, 0)]
    lines = lambda m, e: [ln.rstrip("\n") for ln in PH.lines_of(both(3, sup, votes, m, e), True)]
    assert lines(2, 2) == ["H\t0\t0\t0", "H\t1\t0\t0", "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t3\t0\tforest"]
    assert lines(1, 1) == ["H\t0\t0\t0", "H\t1\t0\t0", "H\t2\t0\t1", "K\t0\t3\t2\t0\t4\t0", "E\t0\t1\t3\t0\tforest", "E\t1\t2\t0\t1\tforest"]
    assert lines(3, 1) == ["H\t0\t0\t0"] and lines(1, 4) == ["H\t0\t0\t0", "H\t1\t1\t0", "H\t2\t2\t0"]


def test_twice_round_a_circle_gives_no_vote():
    """the read of tests/test_allele.py that passes the one site of the circle twice: a fragment of two entries of one bubble"""
    k, seqs = HAND["circle"]
    ug, recs = graph_of(seqs, k)
    read = CIRCLE * 2 + CIRCLE[:8]
    reads = [read.encode(), U.rc_str(read).encode()]
    w = PH.whole(k, ug, recs, reads, min_sup=1)
    assert (w["n_full"], w["n_vote"], w["votes"]) == (4, 0, {})
    frags = A.frag_lines(names_of(reads), w["per"][0]["obs"], 1)
    assert frags == ["F\tr0\t2\t0:2+\t0:2+\n", "F\tr1\t2\t0:2-\t0:2-\n"] and PH.votes_from_f_lines(frags) == ({}, 4, 0)
    text = PH.text(k, 1, 1, 2, True, False, recs, w["sup"], w["head"], w["votes"], w["n_vote"], w["res"]).decode().splitlines()
    assert text == ["#phase\tk=%d\tmin_cnt=1\tmin_sup=1\tmin_link=2" % k, "A\t0\tu1-\tu2-\t0\t4\t0\t2\thom2", "T\t2\t68\t2\t12\t6\t4\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0"]


def test_a_read_through_two_bubbles_votes():
    """the reads of tests/test_allele.py through the two SNPs of TWO: r0 and r1 are the haplotypes (cis), r2 joins one half of each (trans)"""
    ug, recs = graph_of(TWO, 5)
    reads = [r.encode() for r in (TWO[0], TWO[1], U.rc_str(TWO[0][:14] + TWO[1][14:]), TWO[0][:15], TWO[1][12:], TWO[0], TWO[1])]
    for chunk_size in (1 << 28, 40, 1):
        w = PH.whole(5, ug, recs, reads, min_sup=2, min_link=2, chunk_size=chunk_size)
        assert w["votes"] == {(0, 1): [4, 1]} and (w["n_full"], w["n_vote"]) == (12, 5)
        text = PH.text(5, 1, 2, 2, True, False, recs, w["sup"], w["head"], w["votes"], w["n_vote"], w["res"]).decode().splitlines()
        assert text == ["#phase\tk=5\tmin_cnt=1\tmin_sup=2\tmin_link=2", "A\t0\tu2-\tu1-\t2\t4\t0\t0\thet", "A\t1\tu4-\tu5+\t4\t2\t0\t0\thet", "H\t0\t0\t0", "H\t1\t0\t0",
                        "K\t0\t2\t1\t0\t3\t0", "E\t0\t1\t4\t1\tforest", "T\t7\t183\t7\t37\t12\t12\t5\t1\t2\t2\t1\t1\t0\t1\t0\t2"]
        stats = PH.text(5, 1, 2, 2, True, True, recs, w["sup"], w["head"], w["votes"], w["n_vote"], w["res"]).decode().splitlines()
        assert stats == [text[0], text[-1]]


def random_table(rng, n_bubble):
    sup = [rng.choice((HET, HET, HET, HOM, (1, 3, 0, 1), (3, 3, 1, 0))) for _ in range(n_bubble)]
    votes = {}
    for _ in range(rng.randint(0, 3 * n_bubble)):
        i, j = sorted(rng.sample(range(n_bubble), 2))
        votes[(i, j)] = [rng.randint(0, 4), rng.randint(0, 4)]
    return sup, {p: v for p, v in votes.items() if v != [0, 0]}


def test_the_two_solves_agree_on_tiny_random_vote_tables():
    rng = random.Random(32)
    n = dict(edge=0, forest=0, conc=0, disc=0, block=0, single=0, tie=0, not_het=0)
    for it in range(300):
        n_bubble = rng.randint(2, 12)
        sup, votes = random_table(rng, n_bubble)
        m, e = rng.choice((1, 2, 3)), rng.choice((1, 2, 3))
        res = both(n_bubble, sup, votes, m, e)
        obs = PH.obs_of_votes(votes, rng)
        assert PH.votes_flat([obs])[0] == votes
        assert PH.votes_from_f_lines(A.frag_lines(["r%d" % s for s in range(len(obs))], obs, 1))[0] == votes
        # a fragment cut between two chunks at a sequence's edge votes the same
        cut = next((x for x in range(len(obs) // 2, len(obs)) if obs[x][0] != obs[x - 1][0]), len(obs))
        first = obs[cut][0] if cut < len(obs) else 0
        assert PH.votes_flat([obs[:cut], [(o[0] - first,) + o[1:] for o in obs[cut:]]])[0] == votes
        recs = PH.fake_recs(n_bubble)
        full = PH.text(15, 1, m, e, True, False, recs, sup, [0] * 6, votes, 0, res).decode().splitlines(True)
        assert full[0] == "#phase\tk=15\tmin_cnt=1\tmin_sup=%d\tmin_link=%d\n" % (m, e) and full[1:1 + n_bubble] == A.allele_lines(recs, sup, m)
        assert [ln for ln in full if ln[0] in "HKE"] == PH.lines_of(res, True) and len(full) == 2 + n_bubble + len(PH.lines_of(res, True))
        plain = PH.text(15, 1, m, e, False, False, recs, sup, [0] * 6, votes, 0, res).decode().splitlines(True)
        assert plain == [ln for ln in full if ln[0] != "E"]
        n["edge"] += len(res["edges"]); n["block"] += res["stats"]["n_block"]; n["single"] += res["stats"]["n_single"]
        for e_ in res["edges"].values():
            n[e_[2]] += 1
        n["tie"] += sum(1 for c, t in votes.values() if c == t)
        n["not_het"] += sum(1 for s in sup if A.call(s, m) != "het")
    assert n["conc"] >= 30 and n["disc"] >= 20 and min(v for key, v in n.items() if key not in ("conc", "disc")) >= 50, n


def planted(seed):
    rng = random.Random(seed)
    a, b, pos, behind = PH.diploid(rng)
    ug, recs = graph_of([a, b], 15)
    reads = PH.diploid_reads(rng, (a, b), 240)
    return a, b, pos, behind, ug, recs, reads


def test_planted_diploids():
    """k = 15, 3 kb, SNPs 25 to 70 bases apart and once 400, error-free reads of about 250 bases from both haplotypes and both strands: within every
    block h(b) ^ (allele 1 of b is haplotype A's) is constant, the long gap parts two blocks, and no edge is discordant; the votes from the
    records are those from strings alone"""
    for seed in DIPLOID_SEEDS:
        a, b, pos, behind, ug, recs, reads = planted(seed)
        assert len(recs) == len(pos) >= 40
        w = PH.whole(15, ug, recs, reads)
        res = w["res"]
        assert res == PH.by_definition(len(recs), w["sup"], w["votes"])
        # from strings alone: the fragments of by_strings()
        per = A.by_strings(15, ug, recs, reads)
        votes, n_vote = {}, 0
        for got in per:
            n_vote += PH.add_votes(votes, [(i, al) for i, al, full, rev in got if full])
        assert (votes, n_vote) == (w["votes"], w["n_vote"]) and n_vote > 300
        # where each bubble lies and whose allele 1 is
        where, is_a = [], []
        for r in recs:
            s = B.oriented(ug, r[2][0])
            at = [(hap.find(word), hap is a) for hap in (a, b) for word in (s, U.rc_str(s)) if hap.find(word) >= 0]
            assert len(at) == 1
            where.append(at[0][0]); is_a.append(int(at[0][1]))
        st = res["stats"]
        assert st["n_disc"] == 0 and st["n_het"] >= 40 and st["n_block"] >= 2
        for blk in res["blocks"]:
            members = [i for i, n in enumerate(res["nodes"]) if n is not None and n[0] == blk[0]]
            assert len({res["nodes"][i][1] ^ is_a[i] for i in members}) == 1, (seed, blk)
            assert len({where[i] >= behind - 20 for i in members}) == 1, "a block across the long gap"
        sides = [{n[0] for i, n in enumerate(res["nodes"]) if n is not None and (where[i] >= behind - 20) == right} for right in (False, True)]
        assert len(sides[0]) == 1 and len(sides[1]) == 1 and st["n_single"] == 0              # a block on either side of the gap, and no other
        # the text does not depend on the chunks
        text = PH.text(15, 1, 2, 2, True, False, recs, w["sup"], w["head"], w["votes"], w["n_vote"], res)
        for chunk_size in (5000, 1):
            c = PH.whole(15, ug, recs, reads, chunk_size=chunk_size)
            assert PH.text(15, 1, 2, 2, True, False, recs, c["sup"], c["head"], c["votes"], c["n_vote"], c["res"]) == text


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_phase.so exports the names include/yak_amd_phase.h declares, tallies its own kernels and none of the libraries below it; the base
    library's names are still those of tests/golden/libyak_amd_names.txt"""
    import yak_amd
    import yak_amd.allele as allele
    import yak_amd.phase as phase
    from test_abi import declared
    want = declared("yak_amd_phase.h")
    assert want == set(phase.PHASE_H_SYMBOLS)
    assert not want & (declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h") | declared("yak_amd_gfa.h") | declared("yak_amd_path.h") | declared("yak_amd_bubble.h") |
                       declared("yak_amd_allele.h"))
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(phase.PHASE_LIB_PATH) == want and nm(allele.ALLELE_LIB_PATH) == declared("yak_amd_allele.h")
    assert sorted(phase.tally()) == sorted(KERNELS)
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    main_tally = [all_main[i].decode() for i in range(n)]
    assert not [b for b in set(main_tally) | set(allele.tally()) if "k_ph_" in b]
    golden = open(os.path.join(ROOT, "tests", "golden", "libyak_amd_names.txt")).read().split("\n")
    assert sorted(nm(yak_amd.LIB_PATH)) == golden[1:golden.index("# tally")] and main_tally == golden[golden.index("# tally") + 1:-1]
    src = open(os.path.join(ROOT, "yak_amd", "phase", "phase.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and {m for m in re.findall(r"YK_LAUNCH\(([^,]+),", src)} == set(KERNELS)
    assert (C.sizeof(phase.PnodeT), C.sizeof(phase.PpairT), C.sizeof(phase.PedgeT), C.sizeof(phase.PblockT)) == (8, 16, 16, 32)
    assert C.sizeof(phase.PhstatT) == 80 and C.sizeof(phase.PhoptT) == 32
    needed = subprocess.run(["readelf", "-d", phase.PHASE_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert all(so in needed for so in ("libyak_amd_allele.so", "libyak_amd_path.so", "libyak_amd_bubble.so", "libyak_amd_gfa.so", "libyak_amd_walk.so", "libyak_amd.so", "libz", "$ORIGIN"))
    o = phase.PhoptT()
    phase.lib().yakamd_phopt_init(C.byref(o))
    assert (o.min_cnt, o.min_sup, o.min_link, o.edges, o.stats_only, o.chunk_size) == (1, 2, 2, 0, 0, 1 << 28)
    for step in ("phase_step.h", "phase_text.h"):                 # the two headers the model shares with the kernels hold no HIP
        text = open(os.path.join(ROOT, "yak_amd", "phase", step)).read()
        assert "hip_runtime" not in text and "__global__" not in text and "threadIdx" not in text


def test_refusals_need_no_device():
    import yak_amd.phase as phase
    L = phase.lib()
    err = L.yakamd_phase_last_error
    assert L.yakamd_phase_open(-1) is None and b"-1 bubbles" in err()
    assert L.yakamd_phase_open(1 << 31) is None and b"2147483648 bubbles" in err()
    assert L.yakamd_phase_stats(None, None) == -1 and b"no table" in err()
    n_out = (C.c_int64 * 2)(7, 7)
    assert L.yakamd_phase_votes_dev(None, None, 0, n_out) == -1 and b"no table" in err() and list(n_out) == [7, 7]
    assert L.yakamd_phase_solve_dev(None, None, 0, 2, 2) == -1 and b"no table" in err()
    for get in (L.yakamd_phase_pairs_dev, L.yakamd_phase_nodes_dev, L.yakamd_phase_edges_dev, L.yakamd_phase_blocks_dev):
        assert get(None, None, 0) == -1 and b"no table" in err()
    assert L.yakamd_phase_reset(None) == -1
    L.yakamd_phase_close(None)
    assert L.yakamd_phase(None, None, None, None) == -1 and b"no options" in err()
    o = phase.PhoptT()
    for field, value, what in (("min_sup", 0, b"min_sup 0"), ("min_link", 0, b"min_link 0"), ("min_link", -3, b"min_link -3"), ("chunk_size", 0, b"chunk_size 0")):
        L.yakamd_phopt_init(C.byref(o))
        setattr(o, field, value)
        assert L.yakamd_phase(C.byref(o), None, b"reads.fa", b"out.txt") == -1 and what in err(), field
        assert not os.path.exists("out.txt")
    L.yakamd_phopt_init(C.byref(o))
    assert L.yakamd_phase(C.byref(o), None, None, None) == -1 and b"no reads" in err()


def test_the_cli_refuses_the_phase_options(tmp_path):
    """-p, -w or -e without -r, -w or -e without -p, -f or -n with -p: exit 1 and one line on stderr, before the table is looked at"""
    cli = os.path.join(ROOT, "yak_amd", "yak-amd")
    run = lambda a: subprocess.run([cli, "bubbles"] + a + [str(tmp_path / "none.yak")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for a in (["-p"], ["-w", "3"], ["-e"], ["-p", "-e", "-w2"], ["-s", "-p"]):
        r = run(a)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == b"yak-amd bubbles: -p, -w and -e need the reads of -r\n", (a, r.stderr)
    r = run(["-p", "-m", "3"])                                       # the check of -m, -n and -f comes first, and its text stays
    assert r.returncode == 1 and r.stderr == b"yak-amd bubbles: -m, -n and -f need the reads of -r\n"
    for a in (["-w", "3"], ["-e"]):
        r = run(["-r", "reads.fa"] + a)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == b"yak-amd bubbles: -w and -e need the phasing of -p\n", (a, r.stderr)
    for a in (["-f"], ["-n", "2"]):
        r = run(["-r", "reads.fa", "-p"] + a)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == b"yak-amd bubbles: -f and -n do not go with -p, which keeps the fragments on the device\n", (a, r.stderr)
    r = run(["-r", "reads.fa", "-p", "-w", "0"])
    assert r.returncode == 2 and b"is not a readable .yak file" in r.stderr          # the header check of the table comes first, as without -p
    u = subprocess.run([cli, "bubbles"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd bubbles") and b"-p" in u.stderr and b"-w VAL" in u.stderr and u.stdout == b""
