"""The read support of the bubbles' alleles (`yak-amd bubbles -r`) without a GPU: the two restatements of tests/allele_util.py --
from the paths, the steps and the bubble records, and from strings alone -- held to each other on tiny random tables with reads cut from their
sources on both strands and on planted diploid genomes, where every read that spans a site must be a full observation of its own haplotype's
allele and of no other, and to hand-derived cases whose F, A and T lines are written out here, with the invariants include/yak_amd_allele.h
promises.  The tables are made as tests/test_gfa.py makes them.  Last, libyak_amd_allele.so itself: its exports, its own launch tally, the sizes of
its structs, and its refusals, which need no device."""
import ctypes as C
import os
import random
import re
import subprocess

import allele_util as A
import bubble_util as B
import graph_util as U
import path_util as P
from conftest import ROOT
from test_bubble import CIRCLE, HAND, PLANTED_SEEDS
from test_gfa import restated

# two SNPs twelve bases apart at k = 5: two bubbles that share their middle flank u0
TWO = ["GTCGACCCGTTCCATCGTGTGGGAGTAAGA", "GTCGACCCTTTCCATCGTGTAGGAGTAAGA"]
KERNELS = ["k_al_index", "k_al_find<COUNT>", "k_al_find<EMIT>", "k_al_tile_sum", "k_al_tile_scan", "k_al_scan_apply"]


def graph_of(seqs, k, min_cnt=1):
    """(unitigs, bubble records) of the table of the strings"""
    st, ug, links = restated(seqs, k, min_cnt, all_pairs=False)
    recs, bs = B.by_links(k, ug, links)
    assert (recs, bs) == B.by_strings(k, ug)
    return ug, recs


def names_of(reads):
    return ["r%d" % i for i in range(len(reads))]


def both(k, ug, recs, reads, min_sup=2, min_frag=1):
    """flat()'s result with its text as lines: the two restatements, which must agree record by record and in their F and A lines, the invariants,
    and the text in other chunkings"""
    d = A.flat(k, ug, recs, reads)
    A.check_invariants(recs, d)
    per = A.by_strings(k, ug, recs, reads)
    assert per == [[(o[1], o[2] & 1, o[2] >> 1 & 1, o[2] >> 2 & 1) for o in d["obs"] if o[0] == s] for s in range(len(reads))]
    names = names_of(reads)
    text = A.text(k, 1, min_sup, min_frag, True, False, names, recs, d)
    lines = text.decode().splitlines(True)
    frags, alleles = A.by_strings_lines(names, recs, per, min_sup, min_frag)
    assert [ln for ln in lines if ln[0] == "F"] == frags and [ln for ln in lines if ln[0] == "A"] == alleles
    assert lines[0] == "#alleles\tk=%d\tmin_cnt=1\tmin_sup=%d\n" % (k, min_sup) and len(lines) == 2 + len(frags) + len(alleles)
    stats = A.text(k, 1, min_sup, min_frag, True, True, names, recs, d).decode().splitlines(True)
    assert stats == [lines[0], lines[-1]]
    plain = A.text(k, 1, min_sup, min_frag, False, False, names, recs, d).decode().splitlines(True)
    t = lines[-1].split("\t")
    assert plain == [lines[0]] + alleles + ["\t".join(t[:7] + ["0"] + t[8:])]       # without fragments: no F line, and none counted
    # the chunks: the observations and the support of the parts add up to those of the whole, whatever the cut
    for chunk_size in (1, 40):
        obs, n_path, n_step = [], 0, 0
        for part in A.chunks(reads, chunk_size):
            c = A.flat(k, ug, recs, [reads[i] for i in part])
            obs += [(part[o[0]], o[1], o[2], o[3] + n_path) for o in c["obs"]]
            n_path += len(c["paths"]); n_step += len(c["steps"])
        assert obs == d["obs"] and (n_path, n_step) == (len(d["paths"]), len(d["steps"]))
    d["lines"] = [ln.rstrip("\n") for ln in lines]
    return d


def hand(name, reads, **kw):
    k, seqs = HAND[name] if name in HAND else (5, TWO)
    ug, recs = graph_of(seqs, k)
    return both(k, ug, recs, [r.encode() for r in reads], **kw)["lines"][1:]


def test_the_two_restatements_agree_on_tiny_random_tables():
    rng = random.Random(31)
    n = dict(bubble=0, full=0, part=0, rev=0, fwd=0, two=0)
    for it in range(200):
        k = (5, 7)[it % 2]
        a = "".join(rng.choice("ACGT") for _ in range(rng.randint(4 * k, 6 * k)))
        p = rng.randrange(k + 1, len(a) - k - 1)
        seqs = [a, a[:p] + rng.choice([c for c in "ACGT" if c != a[p]]) + a[p + 1:]]
        try:
            ug, recs = graph_of(seqs, k)
        except AssertionError:                                     # a node equal to its own reverse complement's neighbour: not this test's matter
            continue
        reads = P.reads_of(rng, seqs, 8, 1, len(a), sub=0.02, n_rate=0.01, mixed_case=True) + [s.encode() for s in seqs] + [P.rc_bytes(s.encode()) for s in seqs]
        d = both(k, ug, recs, reads, min_sup=rng.choice((1, 2, 3)), min_frag=rng.choice((1, 2)))
        n["bubble"] += len(recs)
        for o in d["obs"]:
            n["full" if o[2] & A.FULL else "part"] += 1
            n["rev" if o[2] & A.REV else "fwd"] += 1
        n["two"] += sum(1 for s in d["sup"] if s[0] and s[1])
    assert n["bubble"] >= 40 and n["full"] > 150 and n["part"] > 100 and n["rev"] > 100 and n["fwd"] > 100 and n["two"] >= 20, n


def test_planted_genomes_every_spanning_read_sees_its_own_haplotype():
    n_full = 0
    kinds = set()
    for k, circular in ((11, False), (15, False), (15, True)):
        haps, want = B.planted(k, 1000, PLANTED_SEEDS[(k, circular)], circular)
        ug, recs = graph_of(haps, k)
        assert len(recs) == len(want)
        # where the allele with its two flanking bases stands, and in which haplotype: the planted variants are a base or a few, so it is one place
        site = {}
        for i, r in enumerate(recs):
            for a in (0, 1):
                w = B.oriented(ug, r[0])[-k] + B.oriented(ug, r[2][a]) + B.oriented(ug, r[1])[k - 1]
                at = [(h, x, len(w)) for h in (0, 1) for word in (w, U.rc_str(w)) for x in A.occurrences(haps[h], word)]
                assert len(at) == 1, "an allele that is not one place of one haplotype"
                site[(i, a)] = at[0]
        rng = random.Random(k)
        cuts = []
        for it in range(60):
            h = it & 1
            ln = rng.randint(2 * k, 8 * k)
            x = rng.randrange(0, len(haps[h]) - ln)
            cuts.append((h, x, ln, it % 3 == 0))
        reads = [(U.rc_str(haps[h][x:x + ln]) if rc else haps[h][x:x + ln]).encode() for h, x, ln, rc in cuts]
        d = both(k, ug, recs, reads)
        for s, (h, x, ln, rc) in enumerate(cuts):
            spanned = sorted((i, a) for (i, a), (hh, at, n) in site.items() if hh == h and x <= at and at + n <= x + ln)
            got = sorted((o[1], o[2] & A.A) for o in d["obs"] if o[0] == s and o[2] & A.FULL)
            assert got == spanned, (k, s)
            n_full += len(got)
        kinds.update(r[6] for r in recs if d["sup"][recs.index(r)][0] and d["sup"][recs.index(r)][1])
    assert n_full > 100 and kinds == set("SEI"), (n_full, kinds)  # sites of every type were spanned in both haplotypes


def test_through_each_arm_forward_and_back():
    """the bubble of tests/test_bubble.py: B 0 u2- u0- u1+ u3+ with u0 = CAGGTCTCA and u1 = TGAGTCCTG.  A read as the strings were given passes
    u3 backwards, an arm, u2: from sink to source, rev; the read with T passes u0 forwards, which is arm 1 = u0- backwards"""
    assert hand("bubble", ["TTCAGGTCTCATG", "TTCAGGACTCATG", "CATGAGACCTGAA", "CATGAGTCCTGAA"]) == [
        "F\tr0\t1\t0:1-", "F\tr1\t1\t0:2-", "F\tr2\t1\t0:1+", "F\tr3\t1\t0:2+",
        "A\t0\tu0-\tu1+\t2\t2\t0\t0\thet",
        "T\t4\t52\t4\t12\t4\t4\t4\t1\t1\t0\t0\t0"]


def test_reads_that_do_not_span():
    """r0 starts inside the arm, r1 ends inside it, r2 has an N behind two nodes of it: three partial observations of allele 1; r3 has the N at
    the site itself and no node of an arm; r4 is the source alone, r5 is shorter than k; r6, in lower case with u for t, spans: the one full"""
    assert hand("bubble", ["GGTCTCATG", "TTCAGGTCT", "TTCAGGTCNCATG", "TTCAGGNCTCATG", "CTCATG", "TTCA", "ttcaggucucaug"]) == [
        "F\tr6\t1\t0:1-",
        "A\t0\tu0-\tu1+\t1\t0\t3\t0\tnone",
        "T\t7\t67\t7\t12\t4\t1\t1\t1\t0\t0\t0\t1"]


def test_a_substitution_or_an_n_inside_the_arm():
    """the arms of eight nodes of two_snps: a changed base or an N between the two sites leaves the arm's first node in one path and its last two
    in the next: two partial observations each, none full"""
    assert hand("two_snps", ["CAGAAAATAGCGACGGACC", "CAGAAAATCGCGACGGACC", "CAGAAAATNGCGACGGACC"]) == [
        "F\tr0\t1\t0:2+",
        "A\t0\tu0+\tu1+\t0\t1\t0\t4\tnone",
        "T\t3\t57\t5\t11\t5\t1\t1\t1\t0\t0\t0\t1"]


def test_a_read_through_two_bubbles():
    """r0 and r1 are the haplotypes, r2 the reverse complement of the first half of one and the second of the other, r3 and r4 span one site each"""
    mix = U.rc_str(TWO[0][:14] + TWO[1][14:])
    reads = [TWO[0], TWO[1], mix, TWO[0][:15], TWO[1][12:]]
    assert hand("two", reads) == [
        "F\tr0\t2\t0:2-\t1:2+", "F\tr1\t2\t0:1-\t1:1+", "F\tr2\t2\t1:1-\t0:2+", "F\tr3\t1\t0:2-", "F\tr4\t1\t1:1+",
        "A\t0\tu2-\tu1-\t1\t3\t0\t0\thom2", "A\t1\tu4-\tu5+\t3\t1\t0\t0\thom1",
        "T\t5\t123\t5\t25\t8\t8\t5\t2\t0\t1\t1\t0"]
    # -n 2: the reads that span both
    assert hand("two", reads, min_frag=2) == [
        "F\tr0\t2\t0:2-\t1:2+", "F\tr1\t2\t0:1-\t1:1+", "F\tr2\t2\t1:1-\t0:2+",
        "A\t0\tu2-\tu1-\t1\t3\t0\t0\thom2", "A\t1\tu4-\tu5+\t3\t1\t0\t0\thom1",
        "T\t5\t123\t5\t25\t8\t8\t3\t2\t0\t1\t1\t0"]


def test_twice_round_a_circle():
    """the circle of 13 bases twice and 8 bases more: the site is passed twice with its flanks and a third time as the path's last step"""
    read = CIRCLE * 2 + CIRCLE[:8]
    assert hand("circle", [read, U.rc_str(read)]) == [
        "F\tr0\t2\t0:2+\t0:2+", "F\tr1\t2\t0:2-\t0:2-",
        "A\t0\tu1-\tu2-\t0\t4\t0\t2\thom2",
        "T\t2\t68\t2\t12\t6\t4\t2\t1\t0\t0\t1\t0"]


def test_min_sup_decides_the_call():
    reads = ["TTCAGGTCTCATG", "TTCAGGACTCATG", "CATGAGACCTGAA"]
    for m, call, tail in ((2, "hom1", "0\t1\t0\t0"), (1, "het", "1\t0\t0\t0"), (3, "none", "0\t0\t0\t1")):
        assert hand("bubble", reads, min_sup=m)[3:] == ["A\t0\tu0-\tu1+\t2\t1\t0\t0\t" + call, "T\t3\t39\t3\t9\t3\t3\t3\t1\t" + tail]


def test_a_graph_without_a_bubble():
    assert hand("tip", ["TTCAGGACTCATG", "CAGGAGG"]) == ["T\t2\t20\t2\t4\t0\t0\t0\t0\t0\t0\t0\t0"]


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_allele.so exports the names include/yak_amd_allele.h declares, tallies its own six kernels and none of the libraries below it, and
    those tally what they did; the base library's names are still those of tests/golden/libyak_amd_names.txt"""
    import yak_amd
    import yak_amd.allele as allele
    import yak_amd.bubble as bubble
    import yak_amd.gfa as gfa
    import yak_amd.path as path
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_allele.h")
    assert want == set(allele.ALLELE_H_SYMBOLS)
    assert not want & (declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h") | declared("yak_amd_gfa.h") | declared("yak_amd_path.h") | declared("yak_amd_bubble.h"))
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(allele.ALLELE_LIB_PATH) == want
    assert nm(path.PATH_LIB_PATH) == declared("yak_amd_path.h") and nm(bubble.BUBBLE_LIB_PATH) == declared("yak_amd_bubble.h")
    assert sorted(allele.tally()) == sorted(KERNELS)
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    main_tally = [all_main[i].decode() for i in range(n)]
    below = set(main_tally) | set(walk.tally()) | set(gfa.tally()) | set(path.tally()) | set(bubble.tally())
    assert not below & set(KERNELS) and not [b for b in below if "k_al_" in b]
    golden = open(os.path.join(ROOT, "tests", "golden", "libyak_amd_names.txt")).read().split("\n")
    assert sorted(nm(yak_amd.LIB_PATH)) == golden[1:golden.index("# tally")] and main_tally == golden[golden.index("# tally") + 1:-1]
    src = open(os.path.join(ROOT, "yak_amd", "allele", "allele.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) == len(KERNELS)
    assert C.sizeof(allele.AobsT) == 16 and C.sizeof(allele.AsupT) == 32 and C.sizeof(allele.AlstatT) == 24 and C.sizeof(allele.AloptT) == 32
    needed = subprocess.run(["readelf", "-d", allele.ALLELE_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert all(so in needed for so in ("libyak_amd_path.so", "libyak_amd_bubble.so", "libyak_amd_gfa.so", "libyak_amd_walk.so", "libyak_amd.so", "libz", "$ORIGIN"))
    o = allele.AloptT()
    allele.lib().yakamd_alopt_init(C.byref(o))
    assert (o.min_cnt, o.min_sup, o.min_frag, o.fragments, o.stats_only, o.chunk_size) == (1, 2, 1, 0, 0, 1 << 28)


def test_refusals_need_no_device():
    import yak_amd.allele as allele
    AL = allele.lib()
    err = AL.yakamd_allele_last_error
    assert AL.yakamd_allele_open(None, None) is None and b"no walk" in err()
    assert AL.yakamd_allele_stats(None, None) == -1 and b"no arm map" in err()
    n_out = (C.c_int64 * 2)(7, 7)
    assert AL.yakamd_allele_obs_dev(None, None, 0, None, 0, None, 0, n_out) == -1 and b"no arm map" in err() and list(n_out) == [7, 7]
    assert AL.yakamd_allele_support_dev(None, None, 0) == -1 and AL.yakamd_allele_reset(None) == -1
    AL.yakamd_allele_close(None)
    assert AL.yakamd_alleles(None, None, None, None) == -1 and b"no options" in err()
    o = allele.AloptT()
    for field, value, what in (("min_sup", 0, b"min_sup 0"), ("min_frag", 0, b"min_frag 0"), ("min_frag", -3, b"min_frag -3"), ("chunk_size", 0, b"chunk_size 0")):
        AL.yakamd_alopt_init(C.byref(o))
        setattr(o, field, value)
        assert AL.yakamd_alleles(C.byref(o), None, b"reads.fa", b"out.txt") == -1 and what in err(), field
    AL.yakamd_alopt_init(C.byref(o))
    assert AL.yakamd_alleles(C.byref(o), None, None, None) == -1 and b"no reads" in err()
    ms = (C.c_double * 5)(*[1.0] * 5)
    AL.yakamd_allele_ms(ms)
    assert list(ms) == [0.0] * 5 == allele.ms()


def test_the_cli_refuses_the_allele_options_without_reads(tmp_path):
    """-m, -n or -f without -r: exit 1 and one line on stderr, before the table is looked at; `bubbles` alone still prints its usage"""
    cli = os.path.join(ROOT, "yak_amd", "yak-amd")
    for a in (["-m", "3"], ["-n2"], ["-f"], ["-s", "-f"], ["-m", "2"]):
        r = subprocess.run([cli, "bubbles"] + a + [str(tmp_path / "none.yak")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == b"yak-amd bubbles: -m, -n and -f need the reads of -r\n", (a, r.stderr)
    r = subprocess.run([cli, "bubbles", "-r", "reads.fa", "-m", "0", str(tmp_path / "none.yak")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"is not a readable .yak file" in r.stderr          # the header check of the table comes first, as without -r
    u = subprocess.run([cli, "bubbles"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd bubbles") and b"-r VAL" in u.stderr and u.stdout == b""
