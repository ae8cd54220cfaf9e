"""Host tier of the table commands (`yak print / cntasm / recount / subtract / isec`): the exports are there, the fixture
(tests/golden/tablecmds.json) regenerates, the reference reproduces it where it is built, and the Python restatement of `print` on the oracle's
getseq -- the checker the GPU tier uses on tables without a stored golden -- equals every stored `print` text."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from conftest import GOLD, ROOT
import gen_golden_tablecmds as G
import tablecmds_util as U

EXPORTS = ["yakamd_kmers_dev", "yakamd_print_dev", "yakamd_propt_init", "yakamd_print"]


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "tablecmds.json")))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, oracle):
    d = str(tmp_path_factory.mktemp("tablecmds"))
    p = G.make_inputs(d)
    G.make_tables(os.path.join(ROOT, "oracle", "yko"), d, p)
    return d, p


def test_exports_are_declared_everywhere():
    import yak_amd
    L = C.CDLL(yak_amd.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "yak_amd.h")).read()
    version_script = open(os.path.join(ROOT, "yak_amd", "csrc", "libyak_amd.map")).read()
    globs = re.search(r"global:([^}]*?)local:", version_script, re.S).group(1)
    pats = [g.strip() for g in globs.replace("\n", " ").split(";") if g.strip()]
    import fnmatch
    for name in EXPORTS:
        assert hasattr(L, name), name + " is not exported by libyak_amd.so"
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/yak_amd.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name + " is not global in libyak_amd.map"
        assert name in yak_amd.YAK_AMD_H_SYMBOLS, name
    assert "yakamd_propt_t" in header


def test_propt_defaults():
    import yak_amd
    L = C.CDLL(yak_amd.LIB_PATH)
    o = yak_amd.PropT(7, 7, 7)
    L.yakamd_propt_init(C.byref(o))
    assert (o.with_counts, o.n_threads, o.batch_bytes) == (0, 4, 256 << 20)
    assert C.sizeof(yak_amd.PropT) == 16


def test_hash64_inv_restatement(oracle):
    O = oracle.lib()
    for k in (5, 15, 21, 27, 31):
        m = (1 << 2 * k) - 1
        for x in [0, 1, m, m >> 1, 0x123456789ABCDEF & m] + [(i * 0x9E3779B97F4A7C15) & m for i in range(1, 200)]:
            assert U.hash64_inv(x, m) == O.yko_hash64_inv(x, m)
            assert O.yko_hash64(U.hash64_inv(x, m), m) == x


def test_inputs_regenerate(gold, inputs):
    d, p = inputs
    assert {n: G.md5(f) for n, f in sorted(p.items())} == gold["inputs"]
    assert {n: G.md5(G.table_path(n, d)) for n in G.MADE_TABLES} == gold["tables"]
    assert sorted(gold["print"]) == sorted(G.PRINT_TABLES) and sorted(gold["cntasm"]) == sorted(G.CNTASM) and sorted(gold["table_cmds"]) == sorted(G.TABLE_CMDS)
    assert any(e["tighten_changes_order"] for e in gold["print"].values())


@pytest.mark.parametrize("name", G.PRINT_TABLES)
def test_oracle_getseq_formatted_equals_stored_print(name, gold, inputs, oracle):
    d, _ = inputs
    e = gold["print"][name]
    fn = G.table_path(name, d)
    with_counts = U.oracle_print(oracle, fn, True)
    assert G.expected(e["counts"], with_counts)
    assert G.expected(e["plain"], U.oracle_print(oracle, fn, False))
    assert with_counts.count(b"\n") == e["kmers"]
    k, pairs = U.file_order_pairs(fn)
    assert (U.lines(pairs, k, True) != with_counts) == e["tighten_changes_order"]
    assert sorted(U.lines(pairs, k, True).splitlines()) == sorted(with_counts.splitlines())


def test_tighten_step_is_visible_in_a_stored_case(gold, inputs, oracle):
    """a listing without yak_ch_tighten differs from the stored one for some table: a print that skipped the step would be caught"""
    d, _ = inputs
    moved = [n for n in G.PRINT_TABLES if not G.expected(gold["print"][n]["counts"], U.oracle_print(oracle, G.table_path(n, d), True, tighten=False))]
    assert "sparse" in moved and set(moved) <= {n for n in G.PRINT_TABLES if gold["print"][n]["tighten_changes_order"]}, moved


def test_digit_classes_of_the_digits_table(inputs):
    d, _ = inputs
    cs = [c for _, c in U.file_order_pairs(G.table_path("digits", d))[1]]
    assert sorted({len(str(c)) for c in cs}) == [1, 2, 3, 4] and 1023 in cs


@pytest.mark.skipif(not os.path.exists(G.REF_YAK), reason="reference binary not built")
def test_reference_reproduces_the_fixture(gold, inputs):
    d, p = inputs
    for name in G.PRINT_TABLES:
        assert G.expected(gold["print"][name]["plain"], G.ref_print(G.REF_YAK, G.table_path(name, d), False)), name
        assert G.expected(gold["print"][name]["counts"], G.ref_print(G.REF_YAK, G.table_path(name, d), True)), name
    for group, cases in (("cntasm", G.CNTASM), ("table_cmds", G.TABLE_CMDS)):
        for name, steps in cases.items():
            assert G.expected(gold[group][name], G.run_case(G.REF_YAK, steps, d, p, os.path.join(d, "ref_" + name + ".yak"))), name
