"""`yak-amd unitigs`, its definition restated twice in tests/graph_util.py and held to itself on oracle-counted tables: the
integer formulation against the brute-force walk over oriented k-mer strings, as sets, and both against hand-derived cases; the identity between open
unitigs, nodes and linked sides on every input; and, without a GPU, the refusals of the new entry points and of the command."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT
import graph_util as U

CLI = os.path.join(ROOT, "yak_amd", "yak-amd")


def genome(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def substituted(g, p):
    return g[:p] + {"A": "C", "C": "G", "G": "T", "T": "A"}[g[p]] + g[p + 1:]


G3000 = genome(3000, 5)
CASES = {
    "genome_k31": (31, [G3000]),
    "bubble_k31": (31, [G3000] * 3 + [substituted(G3000, 1500)]),
    "ac_k5": (5, ["AC" * 30]),
    "acg_k5": (5, ["ACG" * 20]),
    "polya_k5": (5, ["A" * 40]),
    "a_c_t_k5": (5, ["A" * 40 + "C" + "T" * 40]),
    "acgt_k5": (5, ["ACGT" * 15]),
    "dense_k5": (5, [r.decode() for r in U.H.planted(5)]),
    "planted_k21": (21, [r.decode() for r in U.H.planted(21)]),
    "tiny_k3": (3, [genome(40, 7), genome(25, 8)]),
}


@pytest.fixture(scope="module")
def tables(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("graph")
    made = {}

    def get(name):
        if name not in made:
            k, recs = CASES[name]
            data, _ = oracle.count_protocol_mem(U.image([r.encode() for r in recs]), k=k, pre=10, bf_shift=0)
            fn = str(d / (name + ".yak"))
            open(fn, "wb").write(data)
            kk, x, c = U.members(fn)
            assert kk == k
            made[name] = (k, x, c)
        return made[name]
    return get


def restated(tab, min_cnt):
    k, x, c = tab
    recs, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs, min_cnt)
    assert sum(1 for u in ug if not u[3]) == st["n_node"] - st["n_linked_side"] // 2 and st["n_linked_side"] % 2 == 0
    assert sum(u[1] for u in ug) == st["n_node"] and all(len(u[0]) == u[1] + k - 1 for u in ug)
    assert st["n_node"] == sum(map(sum, st["deg"])) and st["n_arc"] == sum((l + r) * st["deg"][l][r] for l in range(5) for r in range(5))
    return recs, st, ug


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("min_cnt", [1, 2])
def test_formulations_agree(tables, name, min_cnt):
    k, x, c = tables(name)
    recs, st, ug = restated((k, x, c), min_cnt)
    assert U.as_sets(k, ug) == U.brute(k, x, c, min_cnt)
    # links are symmetric, and lead to nodes
    for i, r in enumerate(recs):
        for s in (0, 1):
            if r[1 + s] != U.NONE:
                j, t = r[1 + s] >> 1, r[1 + s] & 1
                assert recs[j][1 + t] == (i << 1 | s) and recs[j][3] >= min_cnt and r[3] >= min_cnt
    # open unitigs ascend by their start node's listing index, cycles follow
    pos = {U.canon(U.kmer_str(r[0], k)): i for i, r in enumerate(recs)}
    start = [pos[U.canon(u[0][:k])] for u in ug]
    n_open = sum(1 for u in ug if not u[3])
    assert start[:n_open] == sorted(start[:n_open]) and start[n_open:] == sorted(start[n_open:]) and all(u[3] for u in ug[n_open:])
    for u, i in zip(ug, start):
        assert i <= pos[U.canon(u[0][-k:])] or u[3]


def test_tiny_random_inputs(oracle, tmp_path):
    rng = random.Random(3)
    for it in range(60):
        k = rng.choice((3, 5))
        recs = [genome(rng.randint(k, 30), rng.random()) for _ in range(rng.randint(1, 3))]
        data, _ = oracle.count_protocol_mem(U.image([r.encode() for r in recs]), k=k, pre=10, bf_shift=0)
        fn = str(tmp_path / "t.yak")
        open(fn, "wb").write(data)
        kk, x, c = U.members(fn)
        _, _, ug = restated((k, x, c), 1)
        assert U.as_sets(k, ug) == U.brute(k, x, c, 1), recs


def test_hand_derived_cases(tables):
    k = 31
    _, st, ug = restated(tables("genome_k31"), 1)
    assert len(ug) == 1 and ug[0][1:] == (3000 - k + 1, 3000 - k + 1, 0) and U.canon(ug[0][0]) == U.canon(G3000)
    assert st["deg"][1][1] == 3000 - k - 1 and st["deg"][0][1] + st["deg"][1][0] == 2
    # a bubble: the two nodes next to it have a side of two edges, the two branches hold the k k-mers through the site each
    _, st, ug = restated(tables("bubble_k31"), 1)
    assert len(ug) == 4 and sorted(u[1] for u in ug)[:2] == [k, k] and st["deg"][1][2] + st["deg"][2][1] == 2
    assert sorted(u[2] // u[1] for u in ug) == [1, 3, 4, 4] and not any(u[3] for u in ug)
    # min_cnt above the substituted copy's count removes its branch and rejoins the path
    _, st, ug = restated(tables("bubble_k31"), 2)
    assert len(ug) == 1 and ug[0][1] == 3000 - k + 1 and U.canon(ug[0][0]) == U.canon(G3000) and st["n_node"] == 3000 - k + 1
    recs, st, ug = restated(tables("ac_k5"), 1)
    assert st["n_node"] == 2 and st["n_linked_side"] == 4 and [(len(u[0]), u[3]) for u in ug] == [(6, 1)]
    assert ug[0][0][:4] == ug[0][0][2:] and ug[0][0][:5] == U.kmer_str(recs[0][0], 5)
    recs, st, ug = restated(tables("acg_k5"), 1)
    assert st["n_node"] == 3 and st["n_linked_side"] == 6 and [(len(u[0]), u[3]) for u in ug] == [(7, 1)]
    recs, st, ug = restated(tables("polya_k5"), 1)
    assert st["n_node"] == 1 and recs[0][4] == 0x11 and recs[0][1] == recs[0][2] == U.NONE and ug == [("AAAAA", 1, 36, 0)]
    _, st, ug = restated(tables("a_c_t_k5"), 1)
    assert st["n_node"] == 6 and len(ug) == 2
    _, st, ug = restated(tables("dense_k5"), 1)
    assert st["deg"][4][4] > 50 and st["n_node"] > 400


def test_texts():
    ug = [("ACGTACG", 3, 7, 0), ("AAAAA", 1, 36, 0), ("ACACAC", 2, 5, 1)]
    assert U.fasta_text(ug) == (b">u0\tLN:i:7\tKC:i:7\tkm:f:2.3\tCL:i:0\nACGTACG\n>u1\tLN:i:5\tKC:i:36\tkm:f:36.0\tCL:i:0\nAAAAA\n"
                                b">u2\tLN:i:6\tKC:i:5\tkm:f:2.5\tCL:i:1\nACACAC\n")
    assert U.u_line(ug) == "U\t2\t1\t18\t7\t6\n" and U.u_line([]) == "U\t0\t0\t0\t0\t0\n"
    deg = [[0] * 5 for _ in range(5)]
    deg[1][1], deg[0][1] = 4, 2
    st = dict(n_key=9, n_node=6, n_arc=10, n_linked_side=8, deg=deg)
    assert U.stats_text(5, 2, st, ug) == b"#unitigs\tk=5\tmin_cnt=2\nN\t9\t6\t10\t8\nD\t0\t1\t2\nD\t1\t1\t4\nU\t2\t1\t18\t7\t6\n"


def test_cli_refuses_even_and_long_k_before_any_load(tmp_path):
    """the header is all the command reads of these files: there is no table behind it"""
    for k, what in ((30, b"odd"), (41, b"below 32")):
        fn = str(tmp_path / ("k%d.yak" % k))
        open(fn, "wb").write(b"YAK\2" + struct.pack("<3I", k, 10, 1))
        out = str(tmp_path / "o.fa")
        r = subprocess.run([CLI, "unitigs", "-o", out, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 2 and what in r.stderr and r.stdout == b"" and not os.path.exists(out)


def test_no_cpu_fallback_without_gpu(tmp_path):
    """every new entry point refuses without a gfx950 device; the option defaults and the record sizes are pure host code"""
    import yak_amd
    L = yak_amd.lib()
    o = yak_amd.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    assert (o.min_cnt, o.stats_only, o.n_threads, o.batch_keys) == (1, 0, 8, 1 << 24)
    assert C.sizeof(yak_amd.GnodeT) == 32 and C.sizeof(yak_amd.GstatT) == 232 and C.sizeof(yak_amd.UgoptT) == 24
    if L.yakamd_device_count() > 0:
        return
    out = tmp_path / "o.txt"
    assert L.yakamd_graph_open(None, 1) is None and b"no gfx950" in L.yakamd_last_error()
    assert L.yakamd_unitigs(C.byref(o), None, str(out).encode()) == -1 and b"no gfx950" in L.yakamd_last_error()
    st = yak_amd.GstatT()
    assert L.yakamd_graph_stats(None, C.byref(st)) == -1 and L.yakamd_graph_nodes_dev(None, 0, 1, None, 0) == -1
    L.yakamd_graph_close(None)
    assert not out.exists()
