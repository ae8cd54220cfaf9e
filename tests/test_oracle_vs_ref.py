"""The oracle CLI and library next to what the reference wrote for the same inputs: md5 and size of every .yak the
reference binary or library produced (tests/golden/ref_cli.json, made by tests/gen_golden_ref.py from oracle/_ref,
which `make -C oracle ref` compiles from the reference sources).  The inputs come from tools/yaksynth, seeded."""
import hashlib
import json
import os
import subprocess

import pytest

from conftest import GOLD, ROOT

YKO = os.path.join(ROOT, "oracle", "yko")
SYN = os.path.join(ROOT, "tools", "yaksynth")
REF_GOLD = os.path.join(GOLD, "ref_cli.json")

COMBOS = [["-k31"], ["-k31", "-b20"], ["-k31", "-b25"], ["-k21", "-K50k", "-t3"], ["-k41"], ["-k63", "-b24"],
          ["-k27", "-p12", "-b26"], ["-k31", "-b22", "-H40"]]


def combo_id(args):
    return "".join(args)


def md5_size(fn_or_bytes):
    data = fn_or_bytes if isinstance(fn_or_bytes, bytes) else open(fn_or_bytes, "rb").read()
    return [hashlib.md5(data).hexdigest(), len(data)]


def gold():
    return json.load(open(REF_GOLD))


# the inputs (shared with tests/gen_golden_ref.py, which runs the reference on them)
def cli_reads(tmp_path):
    fq = str(tmp_path / "r.fq")
    subprocess.check_call([SYN, "-n", "4000", "-l", "150", "-g", "20000", "-s", "77", "-o", fq])
    return fq


def two_input_reads(tmp_path):
    f1, f2 = str(tmp_path / "1.fq"), str(tmp_path / "2.fq")
    subprocess.check_call([SYN, "-n", "4000", "-g", "20000", "-s", "5", "-o", f1])
    subprocess.check_call([SYN, "-n", "3000", "-g", "20000", "-s", "5", "-e", "0.01", "-o", f2])
    return [f1, f2]


def cntasm_assemblies(tmp_path):
    fas = []
    for j, e in enumerate((0.0, 0.004, 0.008)):
        fa = str(tmp_path / f"asm{j}.fa")
        subprocess.check_call([SYN, "-a", "-n", "10", "-l", "15000", "-g", "100000", "-s", "9", "-e", str(e), "-N", "0.0002", "-o", fa])
        fas.append(fa)
    return fas


SET_OP_READS = ((9000, 0.004, 17), (4000, 0.02, 17))
CORE_READS = ((9000, 0.004, 17), (6000, 0.01, 17), (5000, 0.006, 18))


def k25_reads(tmp_path, specs):
    fqs = []
    for j, (n, e, s) in enumerate(specs):
        fq = str(tmp_path / f"r{j}.fq")
        subprocess.check_call([SYN, "-n", str(n), "-l", "150", "-g", "50000", "-s", str(s), "-e", str(e), "-o", fq])
        fqs.append(fq)
    return fqs


def k25_tables(tmp_path, specs, want):
    """`count -k25` of each read set by the oracle CLI: the bytes must be the reference's (the inputs of the set operations)"""
    tabs = []
    for j, fq in enumerate(k25_reads(tmp_path, specs)):
        t = str(tmp_path / f"t{j}.yak")
        subprocess.run([YKO, "count", "-k25", "-o", t, fq], check=True, stderr=subprocess.DEVNULL)
        assert md5_size(t) == want[j]
        tabs.append(t)
    return tabs


@pytest.mark.parametrize("args", COMBOS, ids=combo_id)
def test_cli_bytes_identical(args, tmp_path, oracle):
    fq = cli_reads(tmp_path)
    b = str(tmp_path / "b.yak")
    subprocess.run([YKO, "count"] + args + ["-o", b, fq], check=True, stderr=subprocess.DEVNULL)
    assert md5_size(b) == gold()["count"][combo_id(args)]


def test_two_input_files(tmp_path, oracle):
    b = str(tmp_path / "b.yak")
    subprocess.run([YKO, "count", "-b24", "-o", b] + two_input_reads(tmp_path), check=True, stderr=subprocess.DEVNULL)
    assert md5_size(b) == gold()["count_two_files"]


@pytest.mark.parametrize("pre_resize", [0, 1], ids=["plain", "resize_before_merge"])
def test_cntasm_sequence_on_the_oracle_equals_reference_cli(pre_resize, tmp_path, oracle):
    """pins the oracle's shrink / setcnt / merge / tighten (htab.c:102-110, 171-285) on `yak cntasm`
    (main.c:90-161): three assemblies, unique k-mers per sample, merged, shrunk, tightened, dumped"""
    import ctypes as C
    O = oracle.lib()
    fas = cntasm_assemblies(tmp_path)
    K = 21
    oo = oracle.copt(k=K, chunk=1900000000)
    ho = None
    for i, fa in enumerate(fas):
        g1 = O.yko_count_file(fa.encode(), C.byref(oo), None)
        if ho is None:
            ho = g1
            O.yko_ch_shrink(ho, 1, 1); O.yko_ch_setcnt(ho, 1)
        else:
            O.yko_ch_merge(ho, g1, 1, 1, pre_resize)
        if i == len(fas) - 1:
            O.yko_ch_shrink(ho, i + 1, 1023)
    O.yko_ch_tighten(ho)
    assert md5_size(oracle.dump_bytes(ho)) == gold()["cntasm"]["resize_before_merge" if pre_resize else "plain"]
    O.yko_ch_destroy(ho)


@pytest.mark.parametrize("cmd", ["subtract", "isec"])
def test_subtract_isec_sequence_on_the_oracle_equals_reference_cli(cmd, tmp_path, oracle):
    """`yak subtract` / `yak isec` (main.c:217-284) against the oracle's restore + set operation + tighten"""
    O = oracle.lib()
    g = gold()
    tabs = k25_tables(tmp_path, SET_OP_READS, g["set_op_tables"])
    o0, o1 = O.yko_ch_restore(tabs[0].encode()), O.yko_ch_restore(tabs[1].encode())
    (O.yko_ch_subtract if cmd == "subtract" else O.yko_ch_isec)(o0, o1)
    O.yko_ch_tighten(o0)
    assert md5_size(oracle.dump_bytes(o0)) == g[cmd]
    O.yko_ch_destroy(o0); O.yko_ch_destroy(o1)


def restore_core_steps(family, tabs):
    return [(2, tabs[0]), (3, tabs[1])] if family == "triobin" else [(4, tabs[0]), (5, tabs[1]), (6, tabs[2])]


@pytest.mark.parametrize("family", ["triobin", "sexchr"])
def test_restore_core_flag_modes_equal_reference_library(family, tmp_path, oracle):
    """yak_ch_restore_core modes 2-6 (htab.c:396-476) as the reference's own shared library (oracle/_ref/libyakref.so)
    computed them against the oracle's restatement: flag sets ORed into one table"""
    O = oracle.lib()
    g = gold()
    tabs = k25_tables(tmp_path, CORE_READS, g["restore_core_tables"])
    ho = None
    for mode, fn in restore_core_steps(family, tabs):
        ho = O.yko_ch_restore_core(ho, fn.encode(), mode, 2, 5)
        assert ho
    data = oracle.dump_bytes(ho)
    assert md5_size(data) == g["restore_core"][family] and len(data) > 16 + 8 * 1024
    assert O.yko_ch_restore_core(None, tabs[0].encode(), 3, 2, 5) is None or not O.yko_ch_restore_core(None, tabs[0].encode(), 3, 2, 5)
