"""The links between unitigs (`yak-amd unitigs -G`) without a GPU: the two restatements of tests/gfa_util.py -- from the graph's
records and the walk's map, and from the unitigs' strings alone -- held to each other on tiny random tables and to hand-derived cases whose lines
are written out here, with the identities include/yak_amd_gfa.h promises.  The tables are made in this file: the canonical k-mers of a few strings
with their counts, listed ascending (graph_util.graph() takes any listing order), so the numbering of the unitigs can be derived by hand too.
Last, libyak_amd_gfa.so itself: its exports, its own launch tally, and its refusals, which need no device."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np

import gfa_util as G
import graph_util as U
import walk_util as W
from conftest import ROOT


def table_of(seqs, k):
    """(x, c): the canonical k-mers of the strings ascending, and how often each occurs"""
    cnt = {}
    for s in seqs:
        for i in range(len(s) - k + 1):
            c = U.canon(s[i:i + k])
            cnt[c] = cnt.get(c, 0) + 1
    keys = sorted(cnt)
    x = np.array([int("".join(str("ACGT".index(ch)) for ch in s), 4) for s in keys], np.uint64)
    return x, np.array([cnt[s] for s in keys], np.int64)


def restated(seqs, k, min_cnt=1, all_pairs=True):
    """(graph tallies, unitigs, links): both restatements, which must agree, and the identities"""
    x, c = table_of(seqs, k)
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    amap, desc, bases = W.restate(k, recs, min_cnt, ug)
    links = G.links_by_map(k, recs, min_cnt, ug, amap)
    assert links == G.links_by_strings(k, ug)
    if all_pairs:
        assert links == G.links_by_strings(k, ug, all_pairs=True)
    G.check_identities(st, ug, links)
    return st, ug, links


def lines(k, ug, links):
    """the S lines' (name, bases) and the L lines of the GFA text"""
    text = G.gfa_text(k, ug, links).decode().splitlines()
    assert text[0] == "H\tVN:Z:1.0" and len(text) == 1 + len(ug) + len(links)
    return [tuple(ln.split("\t")[1:3]) for ln in text if ln[0] == "S"], [ln for ln in text if ln[0] == "L"]


def test_the_two_restatements_agree_on_tiny_random_tables():
    rng = random.Random(22)
    n_link = n_own_mirror = 0
    degs = [0] * 5
    for it in range(60):
        k = rng.choice((3, 5))
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 30))) for _ in range(rng.randint(1, 3))]
        for min_cnt in (1, 2):
            st, ug, links = restated(seqs, k, min_cnt)
            n_link += len(links)
            n_own_mirror += sum(1 for f, t in links if (t ^ 1, f ^ 1) == (f, t))
            degs = [a + b for a, b in zip(degs, G.end_deg(ug, links))]
    assert n_link > 3000 and n_own_mirror > 10 and all(degs), (n_link, n_own_mirror, degs)


def test_poly_a_is_its_own_neighbour_on_both_sides():
    """A * 9 at k = 5: the one node AAAAA has itself behind both sides and no link as stored"""
    st, ug, links = restated(["A" * 9], 5)
    assert ug == [("AAAAA", 1, 5, 0)] and links == [(0, 0), (1, 1)]
    assert lines(5, ug, links)[1] == ["L\tu0\t+\tu0\t+\t4M", "L\tu0\t-\tu0\t-\t4M"]
    assert G.gfa_text(5, ug, links) == b"H\tVN:Z:1.0\nS\tu0\tAAAAA\tLN:i:5\tKC:i:5\tkm:f:5.0\tcl:i:0\nL\tu0\t+\tu0\t+\t4M\nL\tu0\t-\tu0\t-\t4M\n"
    assert G.stats_text(5, 1, st, ug, links).endswith(b"U\t1\t0\t5\t5\t5\nG\t2\t0\t2\t0\t0\t0\n")


def test_hairpin():
    """a run of ACGT at k = 5: ACGTA and CGTAC; behind CGTAC comes GTACG, its own reverse complement's node, so (u0, +) runs into (u0, -), and
    behind (u0, -) = GTACGT comes ACGTA, the start of (u0, +).  Each of the two lines is its own mirror and stands once"""
    st, ug, links = restated(["ACGT" * 4], 5)
    assert [u[0] for u in ug] == ["ACGTAC"] and links == [(0, 1), (1, 0)]
    assert lines(5, ug, links)[1] == ["L\tu0\t+\tu0\t-\t4M", "L\tu0\t-\tu0\t+\t4M"]
    assert all((t ^ 1, f ^ 1) == (f, t) for f, t in links)


def test_cycles_have_their_two_lines():
    for seq, s in (("AC" * 6, "ACACAC"), ("ACG" * 5, "ACGACGA")):
        st, ug, links = restated([seq], 5)
        assert [(u[0], u[3]) for u in ug] == [(s, 1)] and links == [(0, 0), (1, 1)] and G.end_deg(ug, links) == [0] * 5
        assert lines(5, ug, links)[1] == ["L\tu0\t+\tu0\t+\t4M", "L\tu0\t-\tu0\t-\t4M"]
        assert st["n_arc"] == st["n_linked_side"]                    # every arc of a cycle is a link inside it: the two lines are the + 2 n_cycle
    # a cycle beside an open unitig: the cycle comes last and keeps its two lines
    st, ug, links = restated(["AC" * 6, "AAGGT"], 5)
    assert [u[3] for u in ug] == [0, 1] and links == [(2, 2), (3, 3)]


def test_lone_nodes():
    """AACCG has no neighbour and no link.  AACGT has one: behind it comes ACGTT, its own reverse complement, a hairpin of one node"""
    st, ug, links = restated(["AACCG"], 5)
    assert len(ug) == 1 and links == [] and G.end_deg(ug, links) == [2, 0, 0, 0, 0]
    assert G.gfa_text(5, ug, links) == b"H\tVN:Z:1.0\nS\tu0\tAACCG\tLN:i:5\tKC:i:1\tkm:f:1.0\tcl:i:0\n"
    st, ug, links = restated(["AACGT"], 5)
    assert links == [(0, 1)] and G.end_deg(ug, links) == [1, 1, 0, 0, 0]


def test_bubble():
    """TTCAGG [A|T] CTCATG at k = 5: the flank CCTGAA = revcomp(TTCAGG) forks into the two arms, which join in CTCATG; the arm through A is read
    from its smaller end node as TGAGTCCTG.  The fork lists its arms by the base behind CAGG: A before T.  The right flank ends in TCATG, behind
    which comes CATGA, its own reverse complement's node: one hairpin line more"""
    st, ug, links = restated(["TTCAGGACTCATG", "TTCAGGTCTCATG"], 5)
    seg, L = lines(5, ug, links)
    assert seg == [("u0", "CAGGTCTCA"), ("u1", "TGAGTCCTG"), ("u2", "CTCATG"), ("u3", "CCTGAA")]
    assert L == ["L\tu0\t+\tu2\t+\t4M", "L\tu0\t-\tu3\t+\t4M", "L\tu1\t+\tu3\t+\t4M", "L\tu1\t-\tu2\t+\t4M", "L\tu2\t+\tu2\t-\t4M",
                 "L\tu2\t-\tu0\t-\t4M", "L\tu2\t-\tu1\t+\t4M", "L\tu3\t-\tu1\t-\t4M", "L\tu3\t-\tu0\t+\t4M"]
    assert G.end_deg(ug, links) == [1, 5, 2, 0, 0] and st["n_arc"] - st["n_linked_side"] == 9


def test_tip():
    """TTCAGGACTCATG and the tip CAGGAGG at k = 5: behind TTCAGGA = revcomp(TCCTGAA) come AGGAC.. and the tip AGGAG.., C before G"""
    st, ug, links = restated(["TTCAGGACTCATG", "CAGGAGG"], 5)
    seg, L = lines(5, ug, links)
    assert seg == [("u0", "AGGACTCATG"), ("u1", "AGGAGG"), ("u2", "TCCTGAA")]
    assert L == ["L\tu0\t+\tu0\t-\t4M", "L\tu0\t-\tu2\t+\t4M", "L\tu1\t-\tu2\t+\t4M", "L\tu2\t-\tu0\t+\t4M", "L\tu2\t-\tu1\t+\t4M"]
    assert G.end_deg(ug, links) == [2, 3, 1, 0, 0]                   # the tip's far end and that of the flank have no link


def test_every_canonical_5_mer():
    """all 512 nodes: every side has four neighbours, no link, 512 unitigs of one node, every oriented end has four links"""
    every = ["".join("ACGT"[i >> 2 * j & 3] for j in range(5)) for i in range(1024)]
    st, ug, links = restated(every, 5, all_pairs=False)
    assert len(ug) == 512 and st["n_linked_side"] == 0 and st["n_arc"] == 4096 == len(links)
    assert G.end_deg(ug, links) == [0, 0, 0, 0, 1024] and G.n_keys(ug) == 512
    assert [f for f, _ in links] == [e for e in range(1024) for _ in range(4)]
    # (j, o) through b leads to the node of W[1:] + b, read as that string
    for f, t in links[:64] + links[-64:]:
        s = ug[f >> 1][0] if not f & 1 else U.rc_str(ug[f >> 1][0])
        r = ug[t >> 1][0] if not t & 1 else U.rc_str(ug[t >> 1][0])
        assert s[1:] == r[:4]
    assert [("ACGT".index((ug[t >> 1][0] if not t & 1 else U.rc_str(ug[t >> 1][0]))[4])) for _, t in links[:8]] == [0, 1, 2, 3] * 2


def test_min_cnt_moves_the_links():
    """the arm seen once goes away at min_cnt 2: the bubble closes into the one unitig revcomp(TTCAGGACTCATG), which keeps the hairpin behind TCATG"""
    seqs = ["TTCAGGACTCATG"] * 2 + ["TTCAGGTCTCATG"]
    assert len(restated(seqs, 5, 1)[1]) == 4 and len(restated(seqs, 5, 1)[2]) == 9
    st, ug, links = restated(seqs, 5, 2)
    assert ug == [("CATGAGTCCTGAA", 9, 22, 0)] and links == [(1, 0)]


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_gfa.so exports the names include/yak_amd_gfa.h declares -- its own launch tally only through the three wrappers -- and the two
    libraries below it export and tally what they did; the tally lists this library's kernels without a device"""
    import yak_amd
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_gfa.h")
    assert want == set(gfa.GFA_H_SYMBOLS) and not want & (declared("yak.h") | declared("yak_amd.h") | declared("yak_amd_walk.h"))
    nm = lambda p: {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", p], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm(gfa.GFA_LIB_PATH) == want
    assert nm(walk.WALK_LIB_PATH) == declared("yak_amd_walk.h")
    names = sorted(gfa.tally())
    assert names == sorted(["k_gfa_ends", "k_gfa_links<COUNT>", "k_gfa_links<EMIT>", "k_gfa_tile_sum", "k_gfa_tile_scan", "k_gfa_scan_apply"])
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    below = {all_main[i].decode() for i in range(n)} | set(walk.tally())
    assert not below & set(names) and not [b for b in below if "gfa" in b]      # three tables: the other two are what they were
    src = open(os.path.join(ROOT, "yak_amd", "gfa", "gfa.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) >= len(names)
    assert C.sizeof(gfa.GfastatT) == 88
    needed = subprocess.run(["readelf", "-d", gfa.GFA_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "libyak_amd_walk.so" in needed and "libyak_amd.so" in needed and "$ORIGIN" in needed


def test_refusals_need_no_device():
    import yak_amd.gfa as gfa
    GL = gfa.lib()
    assert GL.yakamd_gfa_open(None, 31) is None and b"no walk" in GL.yakamd_gfa_last_error()
    assert GL.yakamd_gfa_stats(None, None) == -1 and GL.yakamd_gfa_links_dev(None, None, 0) == -1 and b"no links" in GL.yakamd_gfa_last_error()
    GL.yakamd_gfa_close(None)
    assert GL.yakamd_unitigs_gfa(None, None, None) == -1 and b"no options" in GL.yakamd_gfa_last_error()


def test_no_cpu_fallback_without_gpu(tmp_path):
    import yak_amd
    import yak_amd.gfa as gfa
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    out = tmp_path / "o.gfa"
    o = yak_amd.UgoptT()
    yak_amd.lib().yakamd_ugopt_init(C.byref(o))
    assert gfa.lib().yakamd_unitigs_gfa(C.byref(o), None, str(out).encode()) == -1 and b"no gfx950" in gfa.lib().yakamd_gfa_last_error()
    assert not out.exists()
