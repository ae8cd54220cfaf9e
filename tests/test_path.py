"""`yak-amd paths` without a GPU: the two restatements of tests/path_util.py -- the hits from the unitigs' strings alone, and from
the graph's records and the walk's map -- held to each other on tiny random tables with reads cut from their sources, every consecutive pair of
steps to the links of tests/gfa_util.py, and to hand-derived cases whose GAF lines are written out here.  The tables are made as in tests/test_gfa.py.
Last, libyak_amd_path.so itself: its exports, its own launch tally, and its refusals, which need no device."""
import ctypes as C
import os
import random
import re
import subprocess

import gfa_util as G
import graph_util as U
import path_util as P
import walk_util as W
from conftest import ROOT
from test_gfa import table_of

BUBBLE = ["TTCAGGACTCATG", "TTCAGGTCTCATG"]


def restated(seqs, k, reads, min_cnt=1, names=None):
    """everything the restatement says of reads (bytes) on the table of seqs: both hit arrays, which must agree, the chain, the rules, the two texts"""
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    amap, desc, bases = W.restate(k, recs, min_cnt, ug)
    img, off, lens = P.image(reads)
    hits = P.hits_by_strings(k, ug, img)
    assert hits == P.hits_by_ints(k, recs, min_cnt, amap, img)
    paths, steps, tally, spans = P.chain(k, ug, hits, off, lens)
    links = G.links_by_strings(k, ug)
    P.check_rules(k, ug, paths, steps, spans, links)
    names = names or ["r%d" % i for i in range(len(reads))]
    return dict(ug=ug, hits=hits, paths=paths, steps=steps, tally=tally, spans=spans, links=links, off=off, lens=lens,
                gaf=P.gaf_text(k, ug, names, lens, paths, steps).decode(), stats=P.stats_text(k, min_cnt, names, lens, tally).decode())


def features(r):
    """what a fixture shows: a path of two or more steps, a sequence with two or more paths, a - step, a path starting / ending inside a unitig"""
    out = set()
    for p in r["paths"]:
        a, n = p["step_off"], p["n_step"]
        if n >= 2:
            out.add("steps")
        j, o, p0, _ = r["spans"][a]
        if p0 != (0 if o == 0 else r["ug"][j][1] - 1):
            out.add("starts_inside")
        j, o, _, p1 = r["spans"][a + n - 1]
        if p1 != (r["ug"][j][1] - 1 if o == 0 else 0):
            out.add("ends_inside")
    if any(s & 1 for s in r["steps"]):
        out.add("minus")
    if any(t[2] >= 2 for t in r["tally"]):
        out.add("paths")
    return out


def test_the_two_restatements_agree_on_tiny_random_tables():
    rng = random.Random(23)
    seen, n_path, n_step = set(), 0, 0
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        reads = P.reads_of(rng, seqs, 6, 1, 25, sub=0.05, n_rate=0.03, mixed_case=True) + [s.encode() for s in seqs]
        for min_cnt in (1, 2):
            r = restated(seqs, k, reads, min_cnt)
            seen |= features(r)
            n_path += len(r["paths"])
            n_step += len(r["steps"])
            if min_cnt == 1:                                     # a source record lies on the graph from end to end
                for s, t in zip(seqs, r["tally"][6:]):
                    assert t[:3] == (len(s) - k + 1,) * 2 + (1,)
    assert seen == {"steps", "paths", "minus", "starts_inside", "ends_inside"} and n_path > 500 and n_step > 1500, (seen, n_path, n_step)


def test_bubble_through_each_arm_and_back():
    """the unitigs of tests/test_gfa.py's bubble: u0 CAGGTCTCA and u1 TGAGTCCTG the arms, u2 CTCATG, u3 CCTGAA = revcomp(TTCAGG).  A read through the
    arm with T passes u3 backwards, u0, u2; through the arm with A it passes u1 backwards; the reverse complement of a read has its steps reversed
    and flipped"""
    r = restated(BUBBLE, 5, [b"TTCAGGTCTCATG", b"TTCAGGACTCATG", b"CATGAGACCTGAA"])
    assert [u[0] for u in r["ug"]] == ["CAGGTCTCA", "TGAGTCCTG", "CTCATG", "CCTGAA"]
    assert r["gaf"] == ("r0\t13\t0\t13\t+\t<u3>u0>u2\t13\t0\t13\t13\t13\t255\n"
                        "r1\t13\t0\t13\t+\t<u3<u1>u2\t13\t0\t13\t13\t13\t255\n"
                        "r2\t13\t0\t13\t+\t<u2<u0>u3\t13\t0\t13\t13\t13\t255\n")
    assert r["tally"] == [(9, 9, 1, 3)] * 3 and {"steps", "minus"} <= features(r)
    assert r["steps"][6:9] == [s ^ 1 for s in reversed(r["steps"][0:3])]
    assert r["stats"] == "#paths\tk=5\tmin_cnt=1\nS\tr0\t13\t9\t9\t1\t3\nS\tr1\t13\t9\t9\t1\t3\nS\tr2\t13\t9\t9\t1\t3\nT\t3\t39\t27\t27\t3\t9\n"


def test_inside_a_unitig():
    """TCAGGTC: it enters u3 backwards one base in (ps 1) and leaves u0 after its third node of five"""
    r = restated(BUBBLE, 5, [b"TCAGGTC"])
    assert r["gaf"] == "r0\t7\t0\t7\t+\t<u3>u0\t11\t1\t8\t7\t7\t255\n"
    assert {"starts_inside", "ends_inside"} <= features(r)


def test_tip():
    """the unitigs of tests/test_gfa.py's tip: u0 AGGACTCATG, u1 AGGAGG the tip, u2 TCCTGAA.  TTCAGGAGG passes u2 backwards and turns into the tip"""
    r = restated(["TTCAGGACTCATG", "CAGGAGG"], 5, [b"TTCAGGAGG", b"CCTCCTGAA"])
    assert [u[0] for u in r["ug"]] == ["AGGACTCATG", "AGGAGG", "TCCTGAA"]
    assert r["gaf"] == "r0\t9\t0\t9\t+\t<u2>u1\t9\t0\t9\t9\t9\t255\nr1\t9\t0\t9\t+\t<u1>u2\t9\t0\t9\t9\t9\t255\n"


def test_twice_round_a_cycle():
    """(AC)6 at k = 5 is the cycle ACACAC of two nodes: a read of eight k-mers goes round four times, and every wrap starts a new step"""
    r = restated(["AC" * 6], 5, [b"AC" * 6, b"GT" * 6])
    assert [(u[0], u[3]) for u in r["ug"]] == [("ACACAC", 1)]
    assert r["gaf"] == "r0\t12\t0\t12\t+\t>u0>u0>u0>u0\t12\t0\t12\t12\t12\t255\nr1\t12\t0\t12\t+\t<u0<u0<u0<u0\t12\t0\t12\t12\t12\t255\n"
    assert all((a, b) in r["links"] for a, b in zip(r["steps"], r["steps"][1:]) if a == b)


def test_hairpin():
    """a run of ACGT at k = 5 is the unitig ACGTAC, which runs into its own reverse complement and back"""
    r = restated(["ACGT" * 4], 5, [b"ACGTACGTAC"])
    assert [u[0] for u in r["ug"]] == ["ACGTAC"]
    assert r["gaf"] == "r0\t10\t0\t10\t+\t>u0<u0>u0\t10\t0\t10\t10\t10\t255\n"


def test_n_short_absent_and_other_letters():
    """an N cuts a read into two paths; a read shorter than k has no k-mer; a read of absent k-mers has k-mers and no hit; lower case and U are bases"""
    r = restated(BUBBLE, 5, [b"TTCAGGNCTCATG", b"TTCA", b"GGGGGGGG", b"ttcaggucucaug", b""], names=["n", "short", "absent", "rna", "empty"])
    assert r["gaf"] == ("n\t13\t0\t6\t+\t<u3\t6\t0\t6\t6\t6\t255\n"
                        "n\t13\t7\t13\t+\t>u2\t6\t0\t6\t6\t6\t255\n"
                        "rna\t13\t0\t13\t+\t<u3>u0>u2\t13\t0\t13\t13\t13\t255\n")
    assert r["tally"] == [(4, 4, 2, 2), (0, 0, 0, 0), (4, 0, 0, 0), (9, 9, 1, 3), (0, 0, 0, 0)] and "paths" in features(r)
    assert r["hits"][:4] == [P.NONE] * 4 and r["hits"][6] == P.NONE and r["hits"][13] == P.NONE and set(r["hits"][19:28]) == {P.NONE, P.ABSENT}
    assert P.gaf_text(5, r["ug"], ["n", "short", "absent", "rna", "empty"], r["lens"], r["paths"], r["steps"], min_len=7).count(b"\n") == 1


def test_lone_node():
    r = restated(["AACCG"], 5, [b"AACCG", b"CGGTT", b"AACCGG"])
    assert r["gaf"] == "r0\t5\t0\t5\t+\t>u0\t5\t0\t5\t5\t5\t255\nr1\t5\t0\t5\t+\t<u0\t5\t0\t5\t5\t5\t255\nr2\t6\t0\t5\t+\t>u0\t5\t0\t5\t5\t5\t255\n"
    assert r["tally"] == [(1, 1, 1, 1), (1, 1, 1, 1), (2, 1, 1, 1)]
    none = restated(["AACCG"], 5, [b"AACCG"], min_cnt=2)            # a table without a node: every k-mer is absent
    assert none["ug"] == [] and none["gaf"] == "" and none["tally"] == [(1, 0, 0, 0)]


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_path.so exports the names include/yak_amd_path.h declares and nothing else; the three libraries below it export and tally what they
    did; the tally lists this library's kernels without a device"""
    import yak_amd
    import yak_amd.gfa as gfa
    import yak_amd.path as path
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_path.h")
    assert want == set(path.PATH_H_SYMBOLS) and not want & (declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h") | declared("yak_amd_gfa.h"))
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(path.PATH_LIB_PATH) == want
    assert nm(gfa.GFA_LIB_PATH) == declared("yak_amd_gfa.h") and nm(walk.WALK_LIB_PATH) == declared("yak_amd_walk.h")
    names = sorted(path.tally())
    assert names == sorted(["k_path_index", "k_path_hits", "k_path_count", "k_path_tile_scan", "k_path_emit", "k_path_tally"])
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    below = {all_main[i].decode() for i in range(n)} | set(walk.tally()) | set(gfa.tally())
    assert not below & set(names) and not [b for b in below if "path" in b and b.startswith("k_")]
    src = open(os.path.join(ROOT, "yak_amd", "path", "path.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) >= len(names)
    step = open(os.path.join(ROOT, "yak_amd", "path", "path_step.h")).read()
    assert '#include "../gfa/gfa_step.h"' in step and "gf_revcomp(uint64_t" not in step and "gf_hash(uint64_t" not in step      # no third copy
    assert C.sizeof(path.PxstatT) == 32 and C.sizeof(path.PpoptT) == 24
    needed = subprocess.run(["readelf", "-d", path.PATH_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libyak_amd_walk.so" in needed and "libyak_amd.so" in needed and "libyak_amd_gfa.so" not in needed and "$ORIGIN" in needed
    nt4 = (C.c_ubyte * 256).in_dll(main, "seq_nt4_table")          # the bases of the restatement are those of the library
    assert {b for b in range(256) if nt4[b] < 4} == set(P.CODE) and all(nt4[b] == c for b, c in P.CODE.items())


def test_refusals_need_no_device(tmp_path):
    import yak_amd.path as path
    L = path.lib()
    assert L.yakamd_path_open(None, 31) is None and b"no walk" in L.yakamd_path_last_error()
    assert L.yakamd_path_stats(None, None) == -1 and b"no index" in L.yakamd_path_last_error()
    assert L.yakamd_path_hits_dev(None, None, 0, None) == -1 and b"no index" in L.yakamd_path_last_error()
    n_out = (C.c_int64 * 2)()
    assert L.yakamd_path_chain_dev(None, None, 0, None, None, 0, None, 0, None, 0, None, n_out) == -1 and b"no index" in L.yakamd_path_last_error()
    L.yakamd_path_close(None)
    out = tmp_path / "o.gaf"
    assert L.yakamd_paths(None, None, None, None) == -1 and b"no options" in L.yakamd_path_last_error()
    o = path.PpoptT()
    L.yakamd_ppopt_init(C.byref(o))
    assert (o.min_cnt, o.min_len, o.stats_only, o.chunk_size) == (1, 0, 0, 1 << 28)
    o.min_len = -1
    assert L.yakamd_paths(C.byref(o), None, b"x.fa", str(out).encode()) == -1 and b"min_len -1" in L.yakamd_path_last_error() and not out.exists()
    o.min_len, o.chunk_size = 0, 0
    assert L.yakamd_paths(C.byref(o), None, b"x.fa", str(out).encode()) == -1 and b"chunk_size 0" in L.yakamd_path_last_error() and not out.exists()


def test_no_cpu_fallback_without_gpu(tmp_path):
    import yak_amd
    import yak_amd.path as path
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    out = tmp_path / "o.gaf"
    o = path.PpoptT()
    path.lib().yakamd_ppopt_init(C.byref(o))
    assert path.lib().yakamd_paths(C.byref(o), None, b"x.fa", str(out).encode()) == -1 and b"no gfx950" in path.lib().yakamd_path_last_error()
    assert not out.exists()
