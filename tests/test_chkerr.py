"""`yak chkerr` on the device, host tier: the new entry points are exported and declared, the options default as the reference's, the
fixture inputs regenerate bit for bit, (where the reference is built) the reference still writes the stored outputs, and the Python
restatement of te_worker's streak rule (tests/chkerr_util.py) holds on hand-made cases."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLD, ROOT
import chkerr_util as U
import gen_golden_chkerr as G

NEW = ["yakamd_chkerr_lookup_dev", "yakamd_chkerr_streaks_dev", "yakamd_ceopt_init", "yakamd_chkerr"]


def golden():
    return json.load(open(os.path.join(GOLD, "chkerr.json")))


def test_chkerr_entry_points_exported_and_declared():
    import yak_amd
    L = yak_amd.lib()
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(yak_amd.YAK_AMD_H_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "yak_amd.h")).read()
    for n in NEW + ["yakamd_ceopt_t"]:
        assert n in hdr, n


def test_ceopt_defaults():
    import yak_amd
    o = yak_amd.CeoptT()
    yak_amd.lib().yakamd_ceopt_init(C.byref(o))
    assert (o.min_cnt, o.min_streak, o.n_threads, o.chunk_size) == (3, 5, 8, 1000000000)   # chkerr.c:104-106


def test_inputs_regenerate(tmp_path):
    p = G.make_inputs(str(tmp_path))
    assert {n: G.md5(f) for n, f in p.items()} == golden()["inputs"]
    assert max(len(s) for s in open(p["asm.fa"], "rb").read().split(b">")) > 1_000_000


def test_golden_covers_every_case():
    g = golden()
    assert set(g["cases"]) == {"k21", "k41"}
    for ks, case in g["cases"].items():
        assert set(case["out"]) == {"asm.fa:%s" % n for n in G.OPTION_SETS}
        out = case["out"]
        assert out["asm.fa:c0"]["bytes"] > 0                      # absent k-mers are low at -c0
        assert out["asm.fa:c1024"]["text"] != out["asm.fa:default"].get("text")
        assert out["asm.fa:sm1"]["bytes"] > out["asm.fa:s0"]["bytes"]   # the extra line of every sequence


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference not built (make -C oracle ref)")
def test_reference_reproduces_golden(tmp_path):
    g = golden()
    p = G.make_inputs(str(tmp_path))
    for ks, case in g["cases"].items():
        k = int(ks[1:])
        tab = str(tmp_path / ("reads_k%d.yak" % k))
        G.ref_count(G.REF_YAK, k, p["reads.fa"], tab)
        assert G.md5(tab) == case["table_md5"], ks
        for name, opts in g["option_sets"].items():
            assert G.expected(case["out"]["asm.fa:" + name], G.ref_chkerr(G.REF_YAK, tab, p["asm.fa"], opts)), (ks, name)


# ---- te_worker's rule on hand cases ----
N = None


def test_rule_c0_reports_absent_only():
    cnt = [N, N, 0, 0, -1, -1, -1, 0, 5, -1]
    assert U.chkerr_lines(b"s", cnt, 3, 0, 1) == b"s\t2\t7\t3\n"          # the three absent ones; count 0 is not below 0
    assert U.chkerr_lines(b"s", cnt, 3, 1, 1) == b"s\t0\t8\t6\n"          # -c1: counts 0 join them


def test_rule_negative_streak_prints_the_initial_state():
    assert U.chkerr_lines(b"e", [], 21, 3, -1) == b"e\t-20\t0\t0\n"      # an empty record
    assert U.chkerr_lines(b"e", [N] * 5 + [9] * 4, 5, 3, -1) == b"e\t-4\t0\t0\n"
    assert U.chkerr_lines(b"a", [N, N, 9, 1, 9], 3, 3, -1) == b"a\t-2\t0\t0\na\t1\t4\t1\n"
    assert U.chkerr_lines(b"b", [1, 1, 9], 1, 3, -1) == b"b\t0\t2\t2\n"   # k = 1, low at position 0: no extra line
    assert U.chkerr_lines(b"b", [9, 1, 1], 1, 3, -1) == b"b\t0\t0\t0\nb\t1\t3\t2\n"


def test_rule_streak_broken_by_n():
    cnt = [N, N, 1, 1, 1, N, N, N, 1, 1, 1, 1]                             # an N between: two streaks
    assert U.chkerr_lines(b"n", cnt, 3, 3, 3) == b"n\t6\t12\t4\n"
    assert U.chkerr_lines(b"n", cnt, 3, 3, 0) == b"n\t0\t5\t3\nn\t6\t12\t4\n"


def test_rule_streaks_at_start_and_end():
    cnt = [N, N] + [0] * 6 + [7] * 3 + [0] * 5
    assert U.chkerr_lines(b"x", cnt, 3, 3, 4) == b"x\t0\t8\t6\nx\t9\t16\t5\n"
    assert U.chkerr_lines(b"x", cnt, 3, 3, 5) == b"x\t0\t8\t6\n"          # > min_streak, strictly


def test_low_runs_match_rule():
    low = [0xFF, 0xFF, 1, 1, 0, 1, 0xFF, 1, 1, 1]
    assert U.low_runs(low, [0], [len(low)], 1) == [(0, 2, 4, 1), (0, 7, 10, 1)]
    assert U.low_runs(low, [0, 6], [6, 4], -1) == [(0, 2, 4, 1), (0, 5, 6, 1), (1, 1, 4, 1)]


def test_kmer_hash_matches_oracle():
    """the restated hashes against the oracle's C ones (yko_hash64 / yko_hash_long)"""
    from oracle import pyoracle
    L = pyoracle.lib()
    L.yko_hash64.restype = C.c_uint64; L.yko_hash64.argtypes = [C.c_uint64, C.c_uint64]
    L.yko_hash_long.restype = C.c_uint64; L.yko_hash_long.argtypes = [C.POINTER(C.c_uint64)]
    import random
    r = random.Random(7)
    for k in (5, 21, 31):
        s = bytes(r.choice(b"ACGT") for _ in range(k))
        mask = (1 << 2 * k) - 1
        x0 = x1 = 0
        for b in s:
            c = U.NT4[b]
            x0 = (x0 << 2 | c) & mask
            x1 = x1 >> 2 | (3 - c) << 2 * (k - 1)
        assert U.kmer_hash(s, k) == L.yko_hash64(min(x0, x1), mask)
    for k in (32, 41, 63):
        s = bytes(r.choice(b"ACGT") for _ in range(k))
        mask, sh, x = (1 << k) - 1, k - 1, [0, 0, 0, 0]
        for b in s:
            c = U.NT4[b]
            x = [(x[0] << 1 | (c & 1)) & mask, (x[1] << 1 | (c >> 1)) & mask, x[2] >> 1 | (1 - (c & 1)) << sh, x[3] >> 1 | (1 - (c >> 1)) << sh]
        assert U.kmer_hash(s, k) == L.yko_hash_long((C.c_uint64 * 4)(*x))
    for h in (0, 1, 0xFFFFFFFF, 123456789):
        for bits in (2, 3, 10):
            assert U.h2b(h, bits) == L.yko_h2b(h, bits)
