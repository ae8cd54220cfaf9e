"""The device walk of `yak-amd unitigs -g` without a GPU.  tests/walk_util.py restates its three results -- the node -> unitig
map, the descriptors, the bases -- from the strings of graph_util.unitigs(); here that restatement is held to hand-derived cases, and the sequential
model of the kernels (tests/tools/uwalk_model_check.cpp: the doubling rounds, the decision, the scans and the cycles with the very functions of
yak_amd/walk/uwalk_step.h and uwalk_host.h, built with the host compiler under the address and undefined-behaviour sanitizers and run as a program
of its own) to the restatement, byte for byte: FASTA, U line and map; nothing of it is loaded into Python.  Last, libyak_amd_walk.so itself:
its exports, its own launch tally, and its refusal without a GPU."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import graph_util as U
import walk_util as W
from conftest import parse_fastx_image
from test_graph import CASES, ROOT, genome

N = U.NONE


def table(oracle, d, name, img, k):
    data, _ = oracle.count_protocol_mem(img, k=k, pre=10, bf_shift=0)
    fn = str(d / (name + ".yak"))
    open(fn, "wb").write(data)
    kk, x, c = U.members(fn)
    assert kk == k
    return x, c


def restated(k, x, c, min_cnt):
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    return recs, ug, W.restate(k, recs, min_cnt, ug)


# ---- the restatement against hand-derived cases ----
def test_two_node_chain_starts_at_the_smaller_index():
    """AAC -> ACC at k = 3, ACC (the larger x) listed first: R of AAC is linked to L of ACC.  The unitig starts at ACC, the end with the smaller
    index, read away from its unlinked side R: reverse-complemented, GGT, and AAC follows reverse-complemented, GTT"""
    aac, acc = 0b000001, 0b000101
    recs = [(acc, N, 1 << 1 | 0, 4, 0x10), (aac, 0 << 1 | 1, N, 3, 0x01)]
    ug = U.unitigs(3, recs, 1)
    assert ug == [("GGTT", 2, 7, 0)]
    assert W.restate(3, recs, 1, ug) == ([(0, 0 << 1 | 1), (0, 1 << 1 | 1)], [(0, 2, 7, 0 << 1 | 0)], b"GGTT")
    # the other listing order: from AAC as stored
    recs = [(aac, 1 << 1 | 1, N, 3, 0x01), (acc, N, 0 << 1 | 0, 4, 0x10)]
    ug = U.unitigs(3, recs, 1)
    assert W.restate(3, recs, 1, ug) == ([(0, 0), (0, 1 << 1 | 0)], [(0, 2, 7, 0)], b"AACC")


def test_lone_node_and_absent_keys():
    recs = [(0b0001101100, N, N, 1, 0), (0b0000011011, N, N, 7, 0), (0b0000000001, N, N, 2, 0)]     # ACGTA below min_cnt, AACGT, AAAAC
    ug = U.unitigs(5, recs, 2)
    assert W.restate(5, recs, 2, ug) == ([(N, 0), (0, 0), (1, 0)], [(0, 1, 7, 1 << 1), (5, 1, 2, 2 << 1)], b"AACGTAAAAC")
    assert W.stats(5, recs, 2, ug) == dict(n_key=3, n_node=2, n_open=2, n_cycle=0, sum_len=10, max_len=5, n50=5)
    assert W.restate(5, recs, 8, []) == ([(N, 0)] * 3, [], b"") and W.stats(5, recs, 8, [])["n50"] == 0


def test_hand_derived_tables(oracle, tmp_path):
    k = 5
    # (AC)n: two nodes, ACACA and its neighbour GTGTG = canon CACAC, one cycle from the smaller index as stored through R
    x, c = table(oracle, tmp_path, "ac", U.image([r.encode() for r in CASES["ac_k5"][1]]), k)
    recs, ug, (amap, desc, bases) = restated(k, x, c, 1)
    assert len(recs) == 2 and [m[0] for m in amap] == [0, 0] and amap[0] == (0, 0) and amap[1][1] >> 1 == 1
    assert desc == [(0, 2, sum(r[3] for r in recs), 0 << 1 | 1)] and len(bases) == 6 and bases[:4] == bases[2:] and bases[:5].decode() == U.kmer_str(recs[0][0], k)
    assert W.cycle_nodes(ug) == 2
    # (ACG)n: three nodes on one cycle, places 0, 1, 2
    x, c = table(oracle, tmp_path, "acg", U.image([r.encode() for r in CASES["acg_k5"][1]]), k)
    recs, ug, (amap, desc, bases) = restated(k, x, c, 1)
    assert sorted(m[1] >> 1 for m in amap) == [0, 1, 2] and amap[0] == (0, 0) and desc[0][1:] == (3, sum(r[3] for r in recs), 1) and len(bases) == 7
    # poly-A: one node, its own neighbour on both sides, no link: an open unitig of one node as stored
    x, c = table(oracle, tmp_path, "polya", U.image([r.encode() for r in CASES["polya_k5"][1]]), k)
    recs, ug, got = restated(k, x, c, 1)
    assert got == ([(0, 0)], [(0, 1, 36, 0)], b"AAAAA")
    # a bubble: four open unitigs, every node in one place, the two branches of k nodes each
    k = 31
    x, c = table(oracle, tmp_path, "bubble", U.image([r.encode() for r in CASES["bubble_k31"][1]]), k)
    recs, ug, (amap, desc, bases) = restated(k, x, c, 1)
    assert len(desc) == 4 and sorted(d[1] for d in desc)[:2] == [k, k] and not any(d[3] & 1 for d in desc)
    for j, d in enumerate(desc):
        assert sorted(m[1] >> 1 for m in amap if m[0] == j) == list(range(d[1])) and amap[d[3] >> 1][:1] == (j,) and amap[d[3] >> 1][1] >> 1 == 0
        assert d[0] == sum(e[1] + k - 1 for e in desc[:j]) and d[2] == sum(r[3] for r, m in zip(recs, amap) if m[0] == j)
    assert len(bases) == sum(d[1] + k - 1 for d in desc) and [d[3] >> 1 for d in desc] == sorted(d[3] >> 1 for d in desc)
    # every node's k bases stand at its place, as stored or reverse-complemented
    for (x_, _, _, cnt, _), (j, at) in zip(recs, amap):
        s = bases[desc[j][0] + (at >> 1):desc[j][0] + (at >> 1) + k].decode()
        assert s == (U.kmer_str(x_, k) if not at & 1 else U.rc_str(U.kmer_str(x_, k)))


# ---- the sequential model of the kernels against the restatement ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++ on the path: the model of the kernels cannot be built"
    exe = str(tmp_path_factory.mktemp("uwalk") / "uwalk_model_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "tools", "uwalk_model_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def model_equals(program, rf, k, recs, min_cnt, ug):
    """the three outputs of the model on the record file rf; returns (rounds, records of cycle nodes)"""
    amap, desc, bases = W.restate(k, recs, min_cnt, ug)
    out = {}
    for mode in ("fasta", "stats", "map"):
        r = subprocess.run([program, rf, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
        out[mode] = r.stdout
    assert out["fasta"] == U.fasta_text(ug)
    assert out["stats"] == U.u_line(ug).encode()
    body, last = out["map"].rsplit(b"R ", 1)
    assert body == W.map_text(amap, desc)
    rounds, host = (int(v) for v in last.split())
    assert host == W.cycle_nodes(ug)
    return rounds, host


def run_case(program, oracle, d, name, img, k, min_cnt):
    x, c = table(oracle, d, name, img, k)
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    rf = str(d / (name + ".rec"))
    U.record_file(rf, k, min_cnt, recs)
    return ug, model_equals(program, rf, k, recs, min_cnt, ug)


def test_model_on_the_hand_cases(program, oracle, tmp_path):
    kinds = set()
    for name, (k, recs) in sorted(CASES.items()):
        for min_cnt in (1, 2):
            ug, _ = run_case(program, oracle, tmp_path, "%s_c%d" % (name, min_cnt), U.image([r.encode() for r in recs]), k, min_cnt)
            kinds.update(("cycle" if u[3] else "single" if u[1] == 1 else "chain") for u in ug)
    assert kinds == {"cycle", "single", "chain"}
    # the two-node chain and the lone node of the hand-derived tests, records written by hand
    aac, acc = 0b000001, 0b000101
    for i, (k, min_cnt, recs) in enumerate(((3, 1, [(acc, N, 1 << 1 | 0, 4, 0x10), (aac, 0 << 1 | 1, N, 3, 0x01)]),
                                            (3, 1, [(aac, 1 << 1 | 1, N, 3, 0x01), (acc, N, 0 << 1 | 0, 4, 0x10)]),
                                            (5, 2, [(0b0001101100, N, N, 1, 0), (0b0000011011, N, N, 7, 0), (0b0000000001, N, N, 2, 0)]),
                                            (5, 1, []))):
        rf = str(tmp_path / ("hand%d.rec" % i))
        U.record_file(rf, k, min_cnt, recs)
        model_equals(program, rf, k, recs, min_cnt, U.unitigs(k, recs, min_cnt))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257])
def test_model_on_chains(program, oracle, tmp_path, n):
    """one chain of n nodes.  A state L links from its terminal finishes in round floor(log2 L) + 1, and one more round, in which no state
    finishes, ends the ranking"""
    k = 31
    ug, (rounds, host) = run_case(program, oracle, tmp_path, "chain%d" % n, U.image([genome(n + k - 1, 100 + n).encode()]), k, 1)
    assert len(ug) == 1 and ug[0][1] == n and not ug[0][3] and host == 0
    assert rounds == (n - 1).bit_length() + 1


def test_model_on_a_genome_and_reads(program, oracle, synth, tmp_path):
    img = parse_fastx_image(os.path.join(ROOT, "tests", "golden", "inputs", "one3000.fa"))
    ug, (rounds, host) = run_case(program, oracle, tmp_path, "one3000", img, 31, 1)
    assert len(ug) == 1 and ug[0][1] == 3000 - 31 + 1 and rounds == (3000 - 31).bit_length() + 1 and host == 0
    # cycles of two and of three nodes whose listing indices lie among those of two chains
    img = U.image([genome(3000, 31).encode(), b"AC" * 20, genome(500, 5).encode(), b"ACG" * 14])
    ug, (_, host) = run_case(program, oracle, tmp_path, "cycles", img, 31, 1)
    assert sorted((u[1], u[3]) for u in ug) == [(2, 1), (3, 1), (470, 0), (2970, 0)] and [u[3] for u in ug] == [0, 0, 1, 1] and host == 5
    for min_cnt in (1, 3):
        ug, _ = run_case(program, oracle, tmp_path, "reads_c%d" % min_cnt, synth(2000, 150), 31, min_cnt)
        assert len(ug) > 1024 if min_cnt == 1 else len(ug) >= 1        # with the error k-mers: more unitigs than one tile of the device's scan


def test_model_on_tiny_random_tables(program, oracle, tmp_path):
    rng = random.Random(3)
    n_unitig = 0
    for it in range(60):
        k = rng.choice((3, 5))
        recs = [genome(rng.randint(k, 30), rng.random()) for _ in range(rng.randint(1, 3))]
        ug, _ = run_case(program, oracle, tmp_path, "t%d" % it, U.image([r.encode() for r in recs]), k, 1)
        n_unitig += len(ug)
    assert n_unitig > 200


def test_model_reports_broken_links(program, tmp_path):
    """a side that promises a chain whose other end never comes: a message, not a walk without end"""
    recs = [(0, 1 << 1 | 0, N, 5, 1), (5, 0 << 1 | 0, 0 << 1 | 0, 5, 0x11)]
    rf = str(tmp_path / "bad.rec")
    U.record_file(rf, 3, 1, recs)
    r = subprocess.run([program, rf, "fasta"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and b"walk: " in r.stderr


# ---- the library itself, without a GPU ----
def test_library_exports_its_header_and_nothing_else():
    """libyak_amd_walk.so exports the names include/yak_amd_walk.h declares -- its own launch tally only through the three wrappers -- and adds none
    to libyak_amd.so; the tally lists this library's kernels without a device"""
    import re
    import yak_amd
    import yak_amd.walk as walk
    from test_abi import declared
    want = declared("yak_amd_walk.h")
    assert want == set(walk.WALK_H_SYMBOLS) and not want & (declared("yak.h") | declared("yak_amd.h"))
    out = subprocess.run(["nm", "-D", "--defined-only", walk.WALK_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == want
    names = sorted(walk.tally())
    assert names == sorted(["k_uw_init", "k_uw_jump", "k_uw_decide", "k_uw_tile_sum", "k_uw_tile_scan", "k_uw_scan_apply", "k_uw_emit", "k_uw_cyc_flag",
                            "k_uw_cyc_gather", "k_uw_cyc_scatter"])
    main = yak_amd.lib()
    all_main = C.POINTER(C.c_char_p)()
    n = main.yakamd_tally_names(C.byref(all_main))
    assert not {all_main[i].decode() for i in range(n)} & set(names)      # two tables: the other library's is what it was
    src = open(os.path.join(ROOT, "yak_amd", "walk", "walk.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) >= len(names)
    assert C.sizeof(walk.UwstatT) == 72


def test_no_cpu_fallback_without_gpu(tmp_path):
    import yak_amd
    import yak_amd.walk as walk
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    WL = walk.lib()
    out = tmp_path / "o.txt"
    o = yak_amd.UgoptT()
    yak_amd.lib().yakamd_ugopt_init(C.byref(o))
    assert WL.yakamd_uwalk_open(None, 1) is None and b"no gfx950" in WL.yakamd_walk_last_error()
    assert WL.yakamd_unitigs_dev(C.byref(o), None, str(out).encode()) == -1 and b"no gfx950" in WL.yakamd_walk_last_error()
    assert WL.yakamd_uwalk_map_dev(None, None, 0) == -1 and WL.yakamd_uwalk_stats(None, None) == -1
    WL.yakamd_uwalk_close(None)
    assert not out.exists()
