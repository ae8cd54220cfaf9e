"""The cleaning of the unitig graph (`yak-amd clean`) without a GPU: the two restatements of tests/clean_util.py -- from the link
list, the descriptors and the bubble records, and from the unitigs' strings alone -- held to each other, with the report, on the tiny random tables
of tests/test_bubble.py, on a planted genome whose errors must all go and nothing else, and on hand-derived cases whose lines are written out here,
with the invariants include/yak_amd_clean.h promises; the oracle's count / subtract sequence on the drop images must leave the restated set.  The
tables are made as tests/test_gfa.py makes them.  Last, libyak_amd_clean.so itself: its exports, its own launch tally, the sizes of its structs, its
NEEDED entries and its refusals, which need no device, and that libyak_amd.so exports and tallies what it did."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import clean_util as K
import graph_util as U
from conftest import ROOT
from test_bubble import HAND
from test_gfa import table_of

FLANK = "GCGTTCAGG"
# name -> (the strings, pop_pct); k = 5, tip_nodes = 5, min_cnt = 1.  tests/test_clean_model.py and tests/test_gpu_clean.py share them
CASES = {
    "tip": (HAND["tip"][1], 100),
    "tip_long_flank": (HAND["tip_long_flank"][1], 100),
    "siblings": ([FLANK + "AC"] * 2 + [FLANK + "TC"], 100),
    "siblings_equal": ([FLANK + "AC", FLANK + "TC"], 100),
    "three_way_tip": ([FLANK + "ATGTGAG", FLANK + "TTACCCA", FLANK + "CG"], 100),
    "tip_minus": ([FLANK + "AC"] + [FLANK + "TC"] * 2, 100),
    "both_sides": (["GCGTTCAGGACTCATG", "ACAGGACC"], 100),
    "short_alone": (["AACCGT"], 100),
    "bubble31": (["TTCAGGACTCATG"] * 3 + ["TTCAGGTCTCATG"], 100),
    "bubble_equal": (HAND["bubble"][1], 100),
    "pct30": (["TTCAGGACTCATG"] * 3 + ["TTCAGGTCTCATG"], 30),
    "pct40": (["TTCAGGACTCATG"] * 3 + ["TTCAGGTCTCATG"], 40),
    "deletion": (HAND["deletion"][1], 100),
    "circle": (HAND["circle"][1], 100),
    "three_way": (HAND["three_way"][1], 100),
    "arm_forks": (HAND["arm_forks"][1], 100),
    "cycles_and_lone": (HAND["cycles_and_lone"][1], 100),
    "every_5_mer": (HAND["every_5_mer"][1], 100),
}
# (k, seed) at which the planted reads have no chance repeat
PLANTED = ((15, 1), (31, 1))


def cleaned(seqs, k, min_cnt=1, T=None, P=100, max_rounds=8):
    """(the rounds, n_in, n_shrunk, the cleaned set, the report with its T and P lines) with both restatements in every round, and the invariants"""
    T = k if T is None else T
    x, c = table_of(seqs, k)
    done, n_in, n_shrunk, (xo, co) = K.rounds(k, x, c, min_cnt, T, P, max_rounds)
    before, after = K.table_set(k, x, c), K.table_set(k, xo, co)
    assert after <= before, "a k-mer that was not there, or another count"
    assert len(before) - sum(d["round"]["removed"] for d in done) - (n_in - n_shrunk) == len(after)
    for d in done:
        r, s = d["round"], d["stats"]
        assert r["tip_nodes"] + r["pop_nodes"] == r["removed"] == len(d["gone"]) == sum(rec[2] for rec in d["recs"])
        assert len(d["image"]) == r["removed"] + k * len(d["recs"]) and K.as_rows(k, d["recs"])[-1:] == [r_ + (len(d["image"]) - r_[2] - k,) for r_ in d["recs"][-1:]]
        assert s["n_pop"] + s["n_pop_kept"] == r["n_bubble"] and not any(d["ug"][rec[0]][3] for rec in d["recs"]), "a cycle removed"
        cyc = {K.kmer_int(U.canon(u[0][i:i + k])) for u in d["ug"] if u[3] for i in range(u[1])}
        assert not cyc & d["gone"]
    if not done[-1]["gone"]:                                     # cleaning the output again removes nothing
        again = K.rounds(k, xo, co, min_cnt, T, P, 1)[0]
        assert len(again) == 1 and not again[0]["gone"] and again[0]["round"] == done[-1]["round"]
    return done, n_in, n_shrunk, after, K.report(k, min_cnt, T, P, done, n_in, n_shrunk, len(xo), True).decode().splitlines()


def hand(name):
    seqs, P = CASES[name]
    done, n_in, n_shrunk, after, lines = cleaned(seqs, 5, P=P)
    assert lines[0] == "#clean\tk=5\tmin_cnt=1\ttip_nodes=5\tpop_pct=%d" % P
    return done, lines[1:]


def test_the_two_restatements_agree_on_tiny_random_tables():
    """the sixty tables of tests/test_bubble.py and its sixty with a changed copy, at min_cnt 1 and 2"""
    rng = random.Random(26)
    n = dict(tip=0, pop=0, kept=0, rounds=0)

    def run(seqs, k):
        for min_cnt in (1, 2):
            done = cleaned(seqs, k, min_cnt)[0]
            n["tip"] += sum(d["round"]["n_tip"] for d in done); n["pop"] += sum(d["round"]["n_pop"] for d in done)
            n["kept"] += sum(d["stats"]["n_tip_kept"] for d in done); n["rounds"] += len(done) >= 2
    for it in range(60):
        k = rng.choice((3, 5))
        run(["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))], k)
    for it in range(60):
        a = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 30)))
        p = rng.randrange(6, len(a) - 6)
        run([a, a[:p] + rng.choice([ch for ch in "ACGT" if ch != a[p]]) + a[p + 1:]], 5)
    assert n["tip"] > 40 and n["pop"] >= 5 and n["kept"] > 5 and n["rounds"] > 30, n      # every kind of decision was taken; three rounds: arm_forks below


def test_options_switch_tips_and_bubbles_off():
    seqs = CASES["arm_forks"][0]
    assert [d["round"]["removed"] for d in cleaned(seqs, 5, T=0)[0]] == [0]              # the tip stays, so the bubble stays cut
    assert [d["round"]["removed"] for d in cleaned(seqs, 5, P=0)[0]] == [2, 0]           # the tip goes, the bubble stays
    assert [d["round"]["removed"] for d in cleaned(seqs, 5, T=2)[0]] == [0]              # a tip of two nodes is not below 2
    assert [d["round"]["removed"] for d in cleaned(seqs, 5, T=3)[0]] == [2, 5, 0]
    assert [d["round"]["removed"] for d in cleaned(seqs, 5, max_rounds=1)[0]] == [2]
    assert [d["round"]["removed"] for d in cleaned(CASES["bubble31"][0], 5, min_cnt=2)[0]] == [0]   # the weak arm went with the shrink


@pytest.mark.parametrize("k,seed", PLANTED)
def test_planted_errors_all_go_and_nothing_else(k, seed):
    """three copies of a genome of 2 kb and twenty reads with one error each, twelve in the middle (bubbles) and eight near an end (tips): what stays
    is exactly the genome's k-mers with the counts they had, in one unitig, after one round and one more that finds nothing"""
    g, recs = K.planted_reads(k, seed)
    done, n_in, n_shrunk, after, lines = cleaned(recs, k)
    x, c = table_of(recs, k)
    genome = {U.canon(g[i:i + k]) for i in range(len(g) - k + 1)}
    assert len(genome) == len(g) - k + 1
    assert after == {(s, n) for s, n in K.table_set(k, x, c) if s in genome} and len(after) == len(genome)
    assert [(d["round"]["n_tip"], d["round"]["n_pop"]) for d in done] == [(8, 12), (0, 0)] and done[0]["round"]["pop_nodes"] == 12 * k
    assert done[0]["round"]["tip_nodes"] == sum(1 + (5 * i) % (k - 1) for i in (0, 1, 2, 3, 16, 17, 18, 19))
    assert len(done[1]["ug"]) == 1 and {rec[4] & 1 for rec in done[0]["recs"]} == {0, 1}
    assert lines[-1] == "C\t2\t%d\t%d\t%d" % (n_in, n_in, len(genome))


# ---- hand-derived cases: k = 5, tip_nodes = 5 ----
def test_a_tip_is_clipped():
    """TTCAGGACTCATG and CAGGAGG (tests/test_bubble.py): u1 = AGGAGG, 2 nodes, nothing behind u1+ and u2+ behind u1-; the anchor's end u2- also leads
    to u0+ of 6 nodes, no candidate: u1 goes.  u2 = TCCTGAA has 3 nodes and nothing behind u2+, but two links behind u2-: deg(e) == 2, no candidate,
    it stays.  Without u1 the rest is one unitig"""
    done, lines = hand("tip")
    assert lines == ["R\t1\t11\t3\t5\t0\t1\t2\t0\t0\t2", "T\t1\tu1\t2\t2\tu2+", "R\t2\t9\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t11\t11\t9"]
    assert [u[0] for u in done[0]["ug"]] == ["AGGACTCATG", "AGGAGG", "TCCTGAA"] and done[0]["stats"]["n_tip_kept"] == 0
    assert done[0]["image"] == b"AGGAGG\n" and [u[0] for u in done[1]["ug"]] == ["CATGAGTCCTGAA"]
    done, lines = hand("tip_long_flank")
    assert lines == ["R\t1\t14\t3\t5\t0\t1\t2\t0\t0\t2", "T\t1\tu2\t2\t2\tu0-", "R\t2\t12\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t14\t14\t12"]
    assert [u[0] for u in done[1]["ug"]] == ["GCGTTCAGGACTCATG"]


def test_of_two_sibling_tips_the_stronger_stays():
    """GCGTTCAGG with AC behind it twice and TC once: u1 = CAGGTC (kc 2) and u2 = GTCCTG = revcomp(CAGGAC) (kc 4) are both candidates at u0+,
    which leads nowhere else; u2 is stronger and stays, u1 goes.  With AC and TC once each the products are equal and the lower j, u1, stays"""
    done, lines = hand("siblings")
    assert lines == ["R\t1\t9\t3\t4\t0\t1\t2\t0\t0\t2", "T\t1\tu1\t2\t2\tu0-", "R\t2\t7\t1\t0\t0\t0\t0\t0\t0\t0", "C\t2\t9\t9\t7"]
    assert [u[:3] for u in done[0]["ug"]] == [("GCGTTCAGG", 5, 15), ("CAGGTC", 2, 2), ("GTCCTG", 2, 4)] and done[0]["stats"]["n_tip_kept"] == 1
    assert [u[0] for u in done[1]["ug"]] == ["GCGTTCAGGAC"]
    done, lines = hand("siblings_equal")
    assert lines == ["R\t1\t9\t3\t4\t0\t1\t2\t0\t0\t2", "T\t1\tu2\t2\t2\tu0-", "R\t2\t7\t1\t0\t0\t0\t0\t0\t0\t0", "C\t2\t9\t9\t7"]
    assert [u[:3] for u in done[0]["ug"]] == [("GCGTTCAGG", 5, 10), ("CAGGTC", 2, 2), ("GTCCTG", 2, 2)] and [u[0] for u in done[1]["ug"]] == ["GCGTTCAGGTC"]


def test_a_tip_entered_through_its_minus_end():
    """AC once and TC twice: u2 = GTCCTG is the weaker one now; u0+ leads to u2-, so the tip is entered through its '-' end and its linked end is
    u2+"""
    done, lines = hand("tip_minus")
    assert lines == ["R\t1\t9\t3\t4\t0\t1\t2\t0\t0\t2", "T\t1\tu2\t2\t2\tu0-", "R\t2\t7\t1\t0\t0\t0\t0\t0\t0\t0", "C\t2\t9\t9\t7"]
    assert (0, 5) in done[0]["links"] and (4, 1) in done[0]["links"] and [u[:3] for u in done[0]["ug"]][1:] == [("CAGGTC", 2, 4), ("GTCCTG", 2, 2)]


def test_a_tip_on_a_three_way_fork():
    """ATGTGAG, TTACCCA and CG behind GCGTTCAGG: u0+ has three links, two into unitigs of 7 nodes and one into u2 = CGCCTG of 2"""
    done, lines = hand("three_way_tip")
    assert lines == ["R\t1\t21\t4\t6\t0\t1\t2\t0\t0\t2", "T\t1\tu2\t2\t2\tu0-", "R\t2\t19\t3\t4\t0\t0\t0\t0\t0\t0", "C\t2\t21\t21\t19"]
    assert [u[:2] for u in done[0]["ug"]] == [("GCGTTCAGG", 5), ("TGGGTAACCTG", 7), ("CGCCTG", 2), ("CAGGATGTGAG", 7)]
    assert [t for f, t in done[0]["links"] if f == 0] == [6, 5, 3] and len(done[1]["ug"]) == 3


def test_a_short_unitig_linked_on_both_sides_stays():
    """GCGTTCAGGACTCATG and ACAGGACC: u2 = GTCCTG = revcomp(CAGGAC), 2 nodes, has two links on either side and stays; the single nodes ACAGG and
    GGACC hang on it and go, for the other link of their anchor's end leads into a unitig of 5 nodes"""
    done, lines = hand("both_sides")
    assert lines == ["R\t1\t14\t5\t9\t0\t2\t2\t0\t0\t2", "T\t1\tu1\t1\t1\tu2-", "T\t1\tu4\t1\t1\tu2+", "R\t2\t12\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t14\t14\t12"]
    assert done[0]["image"] == b"ACAGG\nGGACC\n" and K.as_rows(5, done[0]["recs"]) == [(1, 1, 1, 1, 5, 0), (4, 1, 1, 1, 4, 6)]


def test_a_whole_sequence_shorter_than_tip_nodes_stays():
    """AACCGT: two nodes, no link, no anchor"""
    done, lines = hand("short_alone")
    assert lines == ["R\t1\t2\t1\t0\t0\t0\t0\t0\t0\t0", "C\t1\t2\t2\t2"]


def test_the_weaker_arm_of_a_bubble_is_popped():
    """TTCAGG [A|T] CTCATG with A three times and T once: B u2- u0- u1+ u3+ with u0 = CAGGTCTCA (kc 5) and u1 = TGAGTCCTG (kc 15); u0 goes and
    u1+ is named as the winner.  pop_pct 30: 100 * 5 * 5 <= 30 * 15 * 5 does not hold, the bubble stays; pop_pct 40: 2500 <= 3000, it goes"""
    done, lines = hand("bubble31")
    assert lines == ["R\t1\t14\t4\t9\t1\t0\t0\t1\t5\t5", "P\t1\tu0\t5\t5\tu1+", "R\t2\t9\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t14\t14\t9"]
    assert done[0]["bubbles"][0][:3] == (5, 6, (1, 2)) and [u[:3] for u in done[1]["ug"]] == [("CATGAGTCCTGAA", 9, 31)]
    done, lines = hand("pct30")
    assert lines == ["R\t1\t14\t4\t9\t1\t0\t0\t0\t0\t0", "C\t1\t14\t14\t14"] and done[0]["stats"]["n_pop_kept"] == 1
    assert hand("pct40")[1] == hand("bubble31")[1]


def test_on_equal_coverage_the_second_arm_is_popped():
    """once each: the arms are equal and a2 = u1+ goes.  In the deletion TTCAGG [A|-] CTCATG the record is B u1- u2- u0+ u3+ with 4 nodes of kc 4
    against 5 of kc 5: the products are equal, and a2 = u0 goes although it has the lower number"""
    done, lines = hand("bubble_equal")
    assert lines == ["R\t1\t14\t4\t9\t1\t0\t0\t1\t5\t5", "P\t1\tu1\t5\t5\tu0-", "R\t2\t9\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t14\t14\t9"]
    done, lines = hand("deletion")
    assert lines == ["R\t1\t13\t4\t9\t1\t0\t0\t1\t5\t5", "P\t1\tu0\t5\t5\tu2-", "R\t2\t8\t1\t1\t0\t0\t0\t0\t0\t0", "C\t2\t13\t13\t8"]
    assert done[0]["bubbles"][0][2:5] == ((5, 0), (4, 5), (4, 5)) and [u[0] for u in done[1]["ug"]] == ["CATGAGCCTGAA"]


def test_a_circle_with_one_snp_becomes_a_cycle():
    done, lines = hand("circle")
    assert lines == ["R\t1\t18\t3\t8\t1\t0\t0\t1\t5\t5", "P\t1\tu2\t5\t5\tu1-", "R\t2\t13\t1\t2\t0\t0\t0\t0\t0\t0", "C\t2\t18\t18\t13"]
    assert [u[1:] for u in done[1]["ug"]] == [(13, 21, 1)]


def test_what_is_no_tip_and_no_simple_bubble_is_untouched():
    """a three-way fork, cycles and a lone node, all 512 canonical 5-mers"""
    assert hand("three_way")[1] == ["R\t1\t18\t7\t18\t0\t0\t0\t0\t0\t0", "C\t1\t18\t18\t18"]
    assert hand("cycles_and_lone")[1] == ["R\t1\t6\t3\t4\t0\t0\t0\t0\t0\t0", "C\t1\t6\t6\t6"]
    assert hand("every_5_mer")[1] == ["R\t1\t512\t512\t4096\t0\t0\t0\t0\t0\t0", "C\t1\t512\t512\t512"]


def test_a_tip_on_a_bubble_arm_takes_three_rounds():
    """the bubble and GGTCTGG leaving the T arm in its middle: round 1 clips u3 = GTCTGG, round 2 sees the bubble whole -- the T arm has kc 6 now,
    the A arm 5 -- and pops u1, round 3 finds one unitig"""
    done, lines = hand("arm_forks")
    assert lines == ["R\t1\t16\t6\t13\t0\t1\t2\t0\t0\t2", "T\t1\tu3\t2\t2\tu0-", "R\t2\t14\t4\t9\t1\t0\t0\t1\t5\t5", "P\t2\tu1\t5\t5\tu0-",
                     "R\t3\t9\t1\t1\t0\t0\t0\t0\t0\t0", "C\t3\t16\t16\t9"]
    assert [u[:3] for u in done[2]["ug"]] == [("CATGAGACCTGAA", 9, 14)]


# ---- the oracle ----
def test_the_oracle_subtracts_the_drop_images_to_the_restated_set(tmp_path):
    """the oracle counts the input into T, shrinks it, and per round counts the drop image into D and subtracts D from T: the dump holds the restated
    surviving set, k-mer for k-mer and count for count"""
    from oracle import pyoracle
    L = pyoracle.lib()
    for name, k, min_cnt, recs in [("planted", 15, 1, K.planted_reads(15, 1)[1]), ("arm_forks", 5, 1, CASES["arm_forks"][0]), ("closing", 5, 2, HAND["closing"][1])]:
        img = U.image([r.encode() for r in recs])
        o = pyoracle.copt(k=k, pre=10)
        t = L.yko_count_mem(img, len(img), C.byref(o), None)
        if min_cnt > 1:
            L.yko_ch_shrink(t, min_cnt, 1023)
        x, c = table_of(recs, k)
        done, n_in, n_shrunk, (xo, co) = K.rounds(k, x, c, min_cnt, k, 100)
        for d in done:
            if not d["gone"]:
                continue
            drop = L.yko_count_mem(d["image"], len(d["image"]), C.byref(o), None)
            assert drop.contents.tot == len(d["gone"])
            L.yko_ch_subtract(t, drop)
            L.yko_ch_destroy(drop)
        fn = str(tmp_path / (name + ".yak"))
        assert L.yko_ch_dump(t, fn.encode()) == 0
        L.yko_ch_destroy(t)
        kk, gx, gc = U.members(fn)
        assert kk == k and K.table_set(k, gx, gc) == K.table_set(k, xo, co) and len(gx) == len(xo)


# ---- the library itself, without a GPU ----
KERNELS = ["k_cln_first", "k_cln_tips", "k_cln_pops", "k_cln_find<COUNT>", "k_cln_find<EMIT>", "k_cln_tile_sum", "k_cln_tile_scan", "k_cln_scan_apply", "k_cln_image"]


def test_library_exports_its_header_and_nothing_else():
    import yak_amd.bubble as bubble
    import yak_amd.clean as clean
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_clean.h")
    below = declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h") | declared("yak_amd_gfa.h") | declared("yak_amd_bubble.h")
    assert want == set(clean.CLEAN_H_SYMBOLS) and not want & below
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(clean.CLEAN_LIB_PATH) == want
    assert nm(bubble.BUBBLE_LIB_PATH) == declared("yak_amd_bubble.h") and nm(gfa.GFA_LIB_PATH) == declared("yak_amd_gfa.h") and nm(walk.WALK_LIB_PATH) == declared("yak_amd_walk.h")
    assert sorted(clean.tally()) == sorted(KERNELS) and not any(clean.tally().values())
    others = set(walk.tally()) | set(gfa.tally()) | set(bubble.tally())
    assert not others & set(KERNELS) and not [b for b in others if "cln" in b]
    src = open(os.path.join(ROOT, "yak_amd", "clean", "clean.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) == len(KERNELS)
    assert C.sizeof(clean.CleanRecT) == 48 and C.sizeof(clean.CleanstatT) == 64 and C.sizeof(clean.CleanroundT) == 72 and C.sizeof(clean.CleanoptT) == 20
    needed = subprocess.run(["readelf", "-d", clean.CLEAN_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert all(so in needed for so in ("libyak_amd_bubble.so", "libyak_amd_gfa.so", "libyak_amd_walk.so", "libyak_amd.so", "$ORIGIN"))
    o = clean.options()
    assert (o.min_cnt, o.tip_nodes, o.pop_pct, o.max_rounds, o.list) == (1, -1, 100, 8, 0)


def test_the_base_library_exports_and_tallies_what_it_did():
    """libyak_amd.so is not part of this layer: its exported names are those of its two headers, as tests/golden/libyak_amd_names.txt lists them with
    the names of its launch tally, and no kernel of the cleaning is among them"""
    import yak_amd
    from test_abi import declared
    L = yak_amd.lib()
    nm = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", yak_amd.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    names = C.POINTER(C.c_char_p)()
    n = L.yakamd_tally_names(C.byref(names))
    tally = [names[i].decode() for i in range(n)]
    want = open(os.path.join(ROOT, "tests", "golden", "libyak_amd_names.txt")).read().split("\n")
    assert sorted(nm) == want[1:want.index("# tally")] and tally == want[want.index("# tally") + 1:-1]
    assert nm == declared("yak.h") | declared("yak_amd.h") and not [t for t in tally if "cln" in t]


def test_refusals_need_no_device():
    import yak_amd.clean as clean
    CL = clean.lib()
    err = CL.yakamd_clean_last_error
    assert CL.yakamd_clean_open(None, None, None, 31, 31, 100) is None and b"no walk" in err()
    assert CL.yakamd_clean_stats(None, None) == -1 and CL.yakamd_clean_records_dev(None, None, 0) == -1 and b"no decisions" in err()
    assert CL.yakamd_clean_image_dev(None, None, 0) == -1 and b"no decisions" in err()
    CL.yakamd_clean_close(None)
    assert CL.yakamd_clean(None, None, None, None) == -1 and b"no options" in err()
    assert CL.yakamd_clean_round(None, None, None) == -1 and b"no options" in err()
    o = clean.options()
    assert CL.yakamd_clean(C.byref(o), None, b"x.yak", None) == -1 and b"not an engine table" in err()
    ms = (C.c_double * 8)(*[1.0] * 8)
    CL.yakamd_clean_ms(ms)
    assert list(ms) == [0.0] * 8 == clean.ms()


def test_no_cpu_fallback_without_gpu(tmp_path):
    import yak_amd
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    from oracle import pyoracle
    img = U.image([s.encode() for s in CASES["tip"][0]])
    fn, out, rep = str(tmp_path / "in.yak"), tmp_path / "out.yak", tmp_path / "r.txt"
    o = pyoracle.copt(k=5, pre=10)
    t = pyoracle.lib().yko_count_mem(img, len(img), C.byref(o), None)
    assert pyoracle.lib().yko_ch_dump(t, fn.encode()) == 0
    pyoracle.lib().yko_ch_destroy(t)
    cli = os.path.join(ROOT, "yak_amd", "yak-amd")
    r = subprocess.run([cli, "clean", "-o", str(rep), fn, str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and r.stdout == b"" and b"no MI355X" in r.stderr and not out.exists() and not rep.exists()
    u = subprocess.run([cli, "clean"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd clean") and u.stdout == b""
    for a in (["-c", "0"], ["-t", "1048577"], ["-b", "101"], ["-r", "0"], ["-r", "65"]):
        r = subprocess.run([cli, "clean"] + a + [fn, str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and b"must be in" in r.stderr and not out.exists(), a
    top = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).stderr.decode()
    assert "      yak-amd clean" in top.split("beyond the reference")[1]
