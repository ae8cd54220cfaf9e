"""`yak sexchr` on the device, host tier: the new entry points are exported and declared, the options default as the reference's, the
fixture inputs regenerate bit for bit, (where the reference is built) the reference still writes the stored output, and the tally
restatement (tests/chkerr_util.py) holds on a hand case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD, ROOT
import chkerr_util as U
import gen_golden_sexchr as G

NEW = ["yakamd_sexchr_reduce_dev", "yakamd_scopt_init", "yakamd_sexchr"]
HEAD = "C\tS  seqName  originalHap  0  #k-mer  #sexchr  #sex1-specifc  #sex2-specific\nC\n"


def golden():
    return json.load(open(os.path.join(GOLD, "sexchr.json")))


def test_sexchr_entry_points_exported_and_declared():
    import yak_amd
    L = yak_amd.lib()
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(yak_amd.YAK_AMD_H_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "yak_amd.h")).read()
    for n in NEW + ["yakamd_scopt_t"]:
        assert n in hdr, n


def test_scopt_defaults():
    import yak_amd
    o = yak_amd.ScoptT()
    yak_amd.lib().yakamd_scopt_init(C.byref(o))
    assert (o.n_threads, o.chunk_size) == (8, 1000000000)          # sexchr.c:13, 113


def test_inputs_regenerate(tmp_path):
    p = G.make_inputs(str(tmp_path))
    assert {n: G.md5(f) for n, f in p.items()} == golden()["inputs"]


def test_golden_has_every_flag_class():
    for ks, case in golden()["cases"].items():
        txt = case["out"]["hap1.fa+hap2.fa"]["text"]
        assert txt.startswith(HEAD)
        rows = [l.split("\t") for l in txt.splitlines()[2:]]
        assert [r[2] for r in rows] == sorted(r[2] for r in rows)       # hap1's records, then hap2's
        assert any(int(r[6]) > 0 for r in rows) and any(int(r[7]) > 0 for r in rows)
        assert any(int(r[4]) > 1_000_000 for r in rows)
        assert ["S", "empty", "1", "0", "0", "0", "0", "0"] in rows


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference not built (make -C oracle ref)")
def test_reference_reproduces_golden(tmp_path):
    g = golden()
    p = G.make_inputs(str(tmp_path))
    for ks, case in g["cases"].items():
        k = int(ks[1:])
        tabs = []
        for t in G.TABLES:
            tabs.append(str(tmp_path / ("%s_k%d.yak" % (t, k))))
            G.ref_count(G.REF_YAK, k, p[t + ".fa"], tabs[-1])
        assert [G.md5(t) for t in tabs] == case["tables_md5"], ks
        assert G.T.expected(case["out"]["hap1.fa+hap2.fa"], G.ref_sexchr(G.REF_YAK, tabs, p["hap1.fa"], p["hap2.fa"])), ks


def test_tally_hand_case():
    f = np.array([0xFF, 0, 1, 2, 3, 7, 0xFF, 1, 0xFF, 0xFF, 4], np.uint8)
    got = U.sexchr_tally(f, [0, 7, 9, 10], [6, 1, 0, 1])
    assert got.tolist() == [[5, 4, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0], [1, 1, 0, 0]]
