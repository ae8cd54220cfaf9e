"""`yak trioeval` on the device, host tier: the new entry points are exported and declared, the options default as the reference's,
the fixture inputs regenerate bit for bit, and (where the reference is built) the reference still writes the stored outputs."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLD, ROOT
import gen_golden_trioeval as G

NEW = ["yakamd_trioeval_reduce_dev", "yakamd_teopt_init", "yakamd_trioeval"]


def golden():
    return json.load(open(os.path.join(GOLD, "trioeval.json")))


def test_trioeval_entry_points_exported_and_declared():
    import yak_amd
    L = yak_amd.lib()
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(yak_amd.YAK_AMD_H_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "yak_amd.h")).read()
    for n in NEW + ["yakamd_teopt_t", "yakamd_streak_t"]:
        assert n in hdr, n


def test_teopt_defaults():
    import yak_amd
    o = yak_amd.TeoptT()
    yak_amd.lib().yakamd_teopt_init(C.byref(o))
    assert (o.min_n, o.print_err, o.print_frag, o.n_threads, o.chunk_size) == (2, 0, 1, 8, 1000000000)   # trioeval.c:13, 163
    assert C.sizeof(yak_amd.StreakT) == 16


def test_inputs_regenerate(tmp_path):
    p = G.make_inputs(str(tmp_path))
    assert {n: G.md5(f) for n, f in p.items()} == golden()["inputs"]


def test_golden_covers_every_case():
    g = golden()
    assert set(g["cases"]) == {"k21", "k41"}
    for case in g["cases"].values():
        assert set(case["out"]) == {"%s:%s" % (fa, n) for fa in G.ASSEMBLIES for n in G.OPTION_SETS}
        assert case["out"]["neither.fa:default"]["text"].endswith("W\t0\t0\t-nan\nH\t0\t0\t-nan\nN\t0\t0\t-nan\n")


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference not built (make -C oracle ref)")
def test_reference_reproduces_golden(tmp_path):
    g = golden()
    p = G.make_inputs(str(tmp_path))
    for ks, case in g["cases"].items():
        k = int(ks[1:])
        tabs = {}
        for who in ("pat", "mat"):
            tabs[who] = str(tmp_path / ("%s_k%d.yak" % (who, k)))
            G.T.ref_count(G.REF_YAK, k, p[who + ".fa"], tabs[who])
            assert G.md5(tabs[who]) == case[who + "_md5"], (ks, who)
        for fa in G.ASSEMBLIES:
            for name, opts in g["option_sets"].items():
                txt = G.ref_trioeval(G.REF_YAK, tabs["pat"], tabs["mat"], p[fa], opts)
                assert G.expected(case["out"]["%s:%s" % (fa, name)], txt), (ks, fa, name)
