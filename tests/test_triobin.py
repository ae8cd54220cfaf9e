"""`yak triobin` on the device, host tier: the new entry points are exported, the fixture inputs regenerate
bit for bit, and (where the reference is built) the reference still writes the stored outputs."""
import json
import os

import pytest

from conftest import GOLD, ROOT
import gen_golden_triobin as G

NEW = ["yakamd_triobin_lookup_dev", "yakamd_triobin_reduce_dev", "yakamd_tbopt_init", "yakamd_triobin"]


def golden():
    return json.load(open(os.path.join(GOLD, "triobin.json")))


def test_triobin_entry_points_exported():
    import yak_amd
    L = yak_amd.lib()
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(yak_amd.YAK_AMD_H_SYMBOLS)


def test_tbopt_defaults():
    import ctypes as C
    import yak_amd
    o = yak_amd.TboptT()
    yak_amd.lib().yakamd_tbopt_init(C.byref(o))
    assert (o.ratio_thres, o.print_diff, o.n_threads, o.chunk_size) == (0.33, 0, 8, 200000000)   # triobin.c:13, 157-159


def test_inputs_regenerate(tmp_path):
    p = G.make_inputs(str(tmp_path))
    assert {n: G.md5(f) for n, f in p.items()} == golden()["inputs"]


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference not built (make -C oracle ref)")
def test_reference_reproduces_golden(tmp_path):
    g = golden()
    p = G.make_inputs(str(tmp_path))
    for ks, case in g["cases"].items():
        k = int(ks[1:])
        tabs = {}
        for who in ("pat", "mat"):
            tabs[who] = str(tmp_path / ("%s_k%d.yak" % (who, k)))
            G.ref_count(G.REF_YAK, k, p[who + ".fa"], tabs[who])
            assert G.md5(tabs[who]) == case[who + "_md5"], (ks, who)
        for name, opts in g["option_sets"].items():
            txt = G.ref_triobin(G.REF_YAK, tabs["pat"], tabs["mat"], p["child.fa"], opts)
            assert G.expected(case["out"][name], txt), (ks, name)
