"""The simple bubbles of the unitig graph (`yak-amd bubbles`) without a GPU: the two restatements of tests/bubble_util.py -- from
the link list and the descriptors, and from the unitigs' strings alone -- held to each other, with both texts, on tiny random tables and on planted
genomes whose variants must all be found with their types, and to hand-derived cases whose lines are written out here, with the invariants
include/yak_amd_bubble.h promises.  The tables are made as tests/test_gfa.py makes them.  Last, libyak_amd_bubble.so itself: its exports, its own
launch tally, the sizes of its structs, and its refusals, which need no device."""
import ctypes as C
import os
import random
import re
import subprocess

import bubble_util as B
import gfa_util as G
import graph_util as U
import hetmer_util as H
from conftest import ROOT
from test_gfa import restated, table_of

# the seeds at which the planted genome of about 1 kb has no chance repeat that hides a variant: (k, circular) -> seed
PLANTED_SEEDS = {(11, False): 2, (11, True): 2, (15, False): 1, (15, True): 1, (31, False): 1, (31, True): 1}
CIRCLE = "ACCAGTCGGATTC"
# name -> (k, the strings); the hand-derived cases below, tests/test_bubble_model.py and tests/test_gpu_bubble.py share them
HAND = {
    "bubble": (5, ["TTCAGGACTCATG", "TTCAGGTCTCATG"]),
    "tip": (5, ["TTCAGGACTCATG", "CAGGAGG"]),
    "tip_long_flank": (5, ["GCGTTCAGGACTCATG", "CAGGAGG"]),
    "closing": (5, ["TTCAGGACTCATG"] * 2 + ["TTCAGGTCTCATG"]),
    "three_way": (5, ["TTCAGGACTCATG", "TTCAGGTCTCATG", "TTCAGGCCTCATG"]),
    "arm_forks": (5, ["TTCAGGACTCATG", "TTCAGGTCTCATG", "GGTCTGG"]),
    "deletion": (5, ["TTCAGGACTCATG", "TTCAGGCTCATG"]),
    "two_snps": (5, ["CAGAAAATAGCGACGGACC", "CAGAAAACAGTGACGGACC"]),
    "circle": (5, [CIRCLE + CIRCLE[:4], CIRCLE[:6] + "A" + CIRCLE[7:] + CIRCLE[:4]]),
    "cycles_and_lone": (5, ["AC" * 6, "ACG" * 5, "AACCG"]),
    "every_5_mer": (5, ["".join("ACGT"[i >> 2 * j & 3] for j in range(5)) for i in range(1024)]),
}


def both(seqs, k, min_cnt=1, strict=False):
    """(graph tallies, unitigs, links, records, stats): both restatements, which must agree, with both texts and the invariants.  The middle
    k-mers of an S bubble differ in the middle base alone, so they are members of one het-mer family; hetmer_util.hetmers() lists a family as a
    pair when it has exactly two members.  strict: every S bubble must be such a pair -- at k = 3 and 5 a third k-mer with the same flanks turns
    up by chance, and then the two must still be of one family"""
    st, ug, links = restated(seqs, k, min_cnt, all_pairs=False)
    recs, bs = B.by_links(k, ug, links)
    recs2, bs2 = B.by_strings(k, ug)
    assert (recs, bs) == (recs2, bs2)
    assert B.text(k, min_cnt, ug, recs) == B.text(k, min_cnt, ug, recs2)
    assert B.stats_text(k, min_cnt, st, ug, links, bs) == B.stats_text(k, min_cnt, st, ug, G.links_by_strings(k, ug), bs2)
    B.check_invariants(k, ug, recs, bs)
    x, c = table_of(seqs, k)
    pairs = {tuple(sorted((U.kmer_str(a, k), U.kmer_str(b, k)))) for a, b, _, _ in H.hetmers(k, x, c, min_cnt)[2]}
    nodes = {U.kmer_str(a, k) for a, n in zip(x, c) if n >= min_cnt}
    for a, b in B.middle_pairs(k, ug, recs):
        family = {U.canon(a[:k // 2] + m + a[k // 2 + 1:]) for m in "ACGT"} & nodes
        assert a != b and {a, b} <= family, "an S bubble whose middle k-mers are not of one het-mer family"
        assert (a, b) in pairs or (len(family) > 2 and not strict), "an S bubble whose middle k-mers are no het-mer pair"
    return st, ug, links, recs, bs


def hand(name, min_cnt=1):
    k, seqs = HAND[name]
    st, ug, links, recs, bs = both(seqs, k, min_cnt, strict=True)
    return ug, recs, bs, B.text(k, min_cnt, ug, recs).decode().splitlines()


def test_the_two_restatements_agree_on_tiny_random_tables():
    rng = random.Random(26)
    n = dict(bubble=0, fork=0, tip=0)
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        for min_cnt in (1, 2):
            bs = both(seqs, k, min_cnt)[4]
            n["bubble"] += bs["n_bubble"]; n["fork"] += bs["n_fork"]; n["tip"] += bs["n_tip"]
    assert n["fork"] > 500 and n["tip"] > 50, n
    # random strings this short hardly ever close a bubble: sixty more at k = 5, each a string of 20 to 30 bases and a copy with one base changed
    for it in range(60):
        k = 5
        a = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 30)))
        p = rng.randrange(6, len(a) - 6)
        seqs = [a, a[:p] + rng.choice([c for c in "ACGT" if c != a[p]]) + a[p + 1:]]
        for min_cnt in (1, 2):
            n["bubble"] += both(seqs, k, min_cnt)[4]["n_bubble"]
    assert n["bubble"] >= 5, n                                   # chance repeats at k = 5 hide most of the sixty


def test_planted_variants_are_all_found_with_their_types():
    kinds = set()
    for (k, circular), seed in sorted(PLANTED_SEEDS.items()):
        seqs, want = B.planted(k, 1000, seed, circular)
        st, ug, links, recs, bs = both(seqs, k, strict=True)
        assert len(want) >= 9 and {w[0] for w in want} == set("SEI")
        assert B.found(recs) == sorted(want), (k, circular)
        assert all(r[5] == 2 for r in recs if r[6] == "E")        # two SNPs, closer than k
        assert all(sorted(len(B.allele(k, ug, a).strip("*")) for a in r[2]) == [0, r[3][0] + r[3][1] - 2 * (k - 1)] for r in recs if r[6] == "I")
        assert bs["n_tip"] == 0 and bs["n_fork"] >= 2 * len(want) and (k == 11 or bs["n_fork"] == 2 * len(want))     # k = 11: one chance fork more
        kinds.update("both" if len({a & 1 for a in r[2]}) == 2 else "+-"[r[2][0] & 1] for r in recs)
        assert both(seqs, k, 2)[4]["n_bubble"] == 0               # every node was seen once or twice: nothing forks at 2
    assert kinds == {"+", "-", "both"}


def test_the_bubble_of_test_gfa():
    """TTCAGG [A|T] CTCATG at k = 5 (the unitigs and links are written out in tests/test_gfa.py): u3 = CCTGAA forks at u3- into u0+ and u1-, and
    both run into u2+; seen from the other side, u2- = CATGAG forks into u0- = TGAGACCTG (through A) and u1+ = TGAGTCCTG (through T), and both
    run into u3+.  The two sides are s = u2- = 5 with t ^ 1 = 7 and s = u3- = 7 with t ^ 1 = 5: the side s = 5 reports.  The flank u3 has two
    nodes, nothing behind u3+ and the fork behind u3-: the one tip.  u2+ has the hairpin behind it, so u2 is none"""
    ug, recs, bs, lines = hand("bubble")
    assert [u[0] for u in ug] == ["CAGGTCTCA", "TGAGTCCTG", "CTCATG", "CCTGAA"]
    assert lines == ["#bubbles\tk=5\tmin_cnt=1", "B\t0\tu2-\tu0-\tu1+\tu3+\tS\t5\t5\t1\t5\t5\tA\tT"]
    assert [B.oriented(ug, a) for a in recs[0][2]] == ["TGAGACCTG", "TGAGTCCTG"]
    assert bs == dict(n_bubble=1, n_type=[1, 0, 0], n_tip=1, tip_nodes=2, max_arm_nodes=5, n_fork=2)
    assert B.stats_line(bs) == b"B\t1\t1\t0\t0\t2\t1\t2\t5\n"


def test_the_tip_of_test_gfa():
    """TTCAGGACTCATG and the tip CAGGAGG at k = 5: u0 = AGGACTCATG, u1 = AGGAGG, u2 = TCCTGAA; u2- forks into u0+ and u1+, and u1+ leads nowhere:
    no bubble, one fork.  u1 (2 nodes, nothing behind u1+, u2+ behind u1-) is the tip; by the definition the flank u2 is one as well: 3 nodes,
    fewer than k, nothing behind u2+ and the fork behind u2-.  With a flank of k nodes or more in its place only the tip is left"""
    ug, recs, bs, lines = hand("tip")
    assert [u[0] for u in ug] == ["AGGACTCATG", "AGGAGG", "TCCTGAA"] and lines == ["#bubbles\tk=5\tmin_cnt=1"]
    assert bs == dict(n_bubble=0, n_type=[0, 0, 0], n_tip=2, tip_nodes=5, max_arm_nodes=0, n_fork=1)
    ug, recs, bs, lines = hand("tip_long_flank")
    assert [u[0] for u in ug] == ["GCGTTCAGGA", "AGGACTCATG", "AGGAGG"] and recs == []
    assert bs == dict(n_bubble=0, n_type=[0, 0, 0], n_tip=1, tip_nodes=2, max_arm_nodes=0, n_fork=1)


def test_min_cnt_2_closes_the_bubble():
    """the arm seen once goes away at min_cnt 2: one unitig, no fork"""
    assert hand("closing", 1)[2]["n_bubble"] == 1
    ug, recs, bs, lines = hand("closing", 2)
    assert len(ug) == 1 and lines == ["#bubbles\tk=5\tmin_cnt=2"] and bs == dict(n_bubble=0, n_type=[0, 0, 0], n_tip=0, tip_nodes=0, max_arm_nodes=0, n_fork=0)
    # the counts of the arms are in the record at min_cnt 1: u1 = revcomp(CAGGACTCA), the arm of the string given twice, has 2 x 5, u0 has 5
    assert hand("closing", 1)[3][1] == "B\t0\tu2-\tu0-\tu1+\tu3+\tS\t5\t5\t1\t5\t10\tA\tT"


def test_a_three_way_fork_is_counted_and_is_no_bubble():
    """A, T and C behind TTCAGG: the flank's end has three links, so has CATGAG's on the other side; GGCCT is its own reverse complement's
    neighbour, which cuts the third arm in two and makes a third fork"""
    ug, recs, bs, lines = hand("three_way")
    assert recs == [] and lines == ["#bubbles\tk=5\tmin_cnt=1"] and bs["n_fork"] == 3 and bs["n_bubble"] == 0


def test_an_arm_that_forks_is_not_simple():
    """the bubble again, and GGTCTGG leaving the arm through T in its middle: that arm is three unitigs now, the ends of the bubble still have two
    links each, and nothing is reported"""
    ug, recs, bs, lines = hand("arm_forks")
    assert len(ug) == 6 and recs == [] and bs["n_fork"] == 3 and bs["n_bubble"] == 0


def test_a_deletion_of_one_base():
    """TTCAGG [A|-] CTCATG: the arm without the base has k - 1 = 4 nodes and no base of its own, the other k = 5 and the one base"""
    ug, recs, bs, lines = hand("deletion")
    assert [u[0] for u in ug] == ["TGAGTCCTG", "CTCATG", "CAGGCTCA", "CCTGAA"]
    assert lines[1:] == ["B\t0\tu1-\tu2-\tu0+\tu3+\tI\t4\t5\t.\t4\t5\t*\tT"]
    assert recs[0][5] is None and bs["n_type"] == [0, 0, 1] and bs["max_arm_nodes"] == 5


def test_two_snps_three_bases_apart():
    """CAGAAAA [T|C] AG [C|T] GACGGACC: one bubble whose arms have k + 3 = 8 nodes and differ in two places"""
    ug, recs, bs, lines = hand("two_snps")
    assert [u[0] for u in ug] == ["AAAACAGTGACG", "AAAATAGCGACG", "CAGAAAA", "GACGGACC"]
    assert lines[1:] == ["B\t0\tu2+\tu0+\tu1+\tu3+\tE\t8\t8\t2\t8\t8\tCAGT\tTAGC"]
    assert bs["n_type"] == [0, 1, 0] and bs["n_tip"] == 2 and bs["tip_nodes"] == 7


def test_a_circular_sequence_with_one_snp():
    """a circle of 13 bases and the same with one base changed, both with their first four bases again behind them: the 8 nodes without the site
    are one open unitig that leaves into the two arms and arrives from them"""
    ug, recs, bs, lines = hand("circle")
    assert [u[0] for u in ug] == ["GGATTCACCAGT", "ATCCTACTG", "ATCCGACTG"]
    assert lines[1:] == ["B\t0\tu0+\tu1-\tu2-\tu0+\tS\t5\t5\t1\t5\t5\tA\tC"]
    assert recs[0][0] >> 1 == recs[0][1] >> 1 == 0 and bs["n_fork"] == 2 and bs["n_tip"] == 0


def test_cycles_and_lone_nodes_have_nothing():
    ug, recs, bs, lines = hand("cycles_and_lone")
    assert [u[3] for u in ug] == [0, 1, 1] and lines == ["#bubbles\tk=5\tmin_cnt=1"]
    assert bs == dict(n_bubble=0, n_type=[0, 0, 0], n_tip=0, tip_nodes=0, max_arm_nodes=0, n_fork=0)


def test_every_canonical_5_mer():
    """512 unitigs of one node, every oriented end with four links: 1024 forks, no end with two"""
    ug, recs, bs, lines = hand("every_5_mer")
    assert len(ug) == 512 and bs == dict(n_bubble=0, n_type=[0, 0, 0], n_tip=0, tip_nodes=0, max_arm_nodes=0, n_fork=1024)


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_bubble.so exports the names include/yak_amd_bubble.h declares -- its own launch tally only through the three wrappers -- and the
    three libraries below it export and tally what they did; the tally lists this library's kernels without a device"""
    import yak_amd
    import yak_amd.bubble as bubble
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_bubble.h")
    assert want == set(bubble.BUBBLE_H_SYMBOLS) and not want & (declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h") | declared("yak_amd_gfa.h"))
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(bubble.BUBBLE_LIB_PATH) == want
    assert nm(gfa.GFA_LIB_PATH) == declared("yak_amd_gfa.h") and nm(walk.WALK_LIB_PATH) == declared("yak_amd_walk.h")
    names = sorted(bubble.tally())
    assert names == sorted(["k_bub_first", "k_bub_find<COUNT>", "k_bub_find<EMIT>", "k_bub_tile_sum", "k_bub_tile_scan", "k_bub_scan_apply", "k_bub_classify"])
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    below = {all_main[i].decode() for i in range(n)} | set(walk.tally()) | set(gfa.tally())
    assert not below & set(names) and not [b for b in below if "bub" in b]      # four tables: the other three are what they were
    src = open(os.path.join(ROOT, "yak_amd", "bubble", "bubble.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) >= len(names)
    assert C.sizeof(bubble.BubbleT) == 80 and C.sizeof(bubble.BubstatT) == 64
    needed = subprocess.run(["readelf", "-d", bubble.BUBBLE_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert all(so in needed for so in ("libyak_amd_gfa.so", "libyak_amd_walk.so", "libyak_amd.so", "$ORIGIN"))


def test_refusals_need_no_device():
    import yak_amd.bubble as bubble
    BL = bubble.lib()
    assert BL.yakamd_bubble_open(None, None, 31) is None and b"no walk" in BL.yakamd_bubble_last_error()
    assert BL.yakamd_bubble_stats(None, None) == -1 and BL.yakamd_bubble_records_dev(None, None, 0) == -1 and b"no bubbles" in BL.yakamd_bubble_last_error()
    BL.yakamd_bubble_close(None)
    assert BL.yakamd_bubbles(None, None, None) == -1 and b"no options" in BL.yakamd_bubble_last_error()
    ms = (C.c_double * 5)(*[1.0] * 5)
    BL.yakamd_bubble_ms(ms)
    assert list(ms) == [0.0] * 5 == bubble.ms()


def test_no_cpu_fallback_without_gpu(tmp_path):
    import yak_amd
    import yak_amd.bubble as bubble
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    out = tmp_path / "o.txt"
    o = yak_amd.UgoptT()
    yak_amd.lib().yakamd_ugopt_init(C.byref(o))
    assert bubble.lib().yakamd_bubbles(C.byref(o), None, str(out).encode()) == -1 and b"no gfx950" in bubble.lib().yakamd_bubble_last_error()
    assert not out.exists()
    cli = os.path.join(ROOT, "yak_amd", "yak-amd")
    u = subprocess.run([cli, "bubbles"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd bubbles") and u.stdout == b""
    top = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).stderr.decode()
    assert "      yak-amd bubbles" in top.split("beyond the reference")[1]
