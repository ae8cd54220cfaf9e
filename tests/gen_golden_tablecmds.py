"""Fixtures of the table commands `yak print / cntasm / recount / subtract / isec` (tests/golden/tablecmds.json).

The inputs are the reference-made tables committed under tests/golden/*.yak, the three assemblies of
test_oracle_vs_ref.cntasm_assemblies and three of its k = 25 tables of reads of one genome (tools/yaksynth, seeded; the tables by the
oracle's CLI, their bytes pinned to the reference's by tests/golden/ref_cli.json) and two files written here from the seeded splitmix64 stream of
gen_golden_triobin: digits.fa, whose `count -k21` table holds counts of one, two, three and four digits up to the saturated 1023, and
digits_half.fa, a part of it (the sequences `recount` counts); and sparse.fq (yaksynth), whose table yak_ch_tighten really resizes.

Run as a script (where the reference is built, `make -C oracle ref`) it stores md5 and size of what the reference writes for every
case, the text itself where it is short, and the md5 of every generated input.
"""
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile

import gen_golden_triobin as T
import tablecmds_util as U
import test_oracle_vs_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))
REF_YAK = T.REF_YAK
GOLD = os.path.join(HERE, "golden")
GOLDEN = os.path.join(GOLD, "tablecmds.json")

SEED = 0x7AB1EC
TEXT_MAX = 4096
PRINT_TABLES = ("nb_k15_fa", "nb_k21", "nb_k27_p12", "nb_k31", "b19_k31", "polyA", "one_read", "edge_fx", "digits", "sparse")
REFUSED_TABLES = ("nb_k32", "nb_k41", "b24_k63_fa")          # k >= 32: the reference has no listing of them (htab.c:359)
# the tables made for the purpose: `count` arguments and input.  sparse: reads at a coverage near one counted without a working filter and
# shrunk to counts >= 2 (main.c:53-58), which leaves sub-tables filled to less than a third -- the ones yak_ch_tighten resizes
MADE_TABLES = {"digits": (["-k21"], "digits.fa"), "sparse": (["-k21", "-b15"], "sparse.fq")}
# a case is a list of command lines; @OUT@ is the case's output file, @A0@ .. the assemblies, @T0@ .. the k = 25 tables of reads of one genome,
# @digits@ / @name@ a table, @half@ digits_half.fa
CNTASM = {
    "plain": [["cntasm", "-k21", "-o", "@OUT@", "@A0@", "@A1@", "@A2@"]],
    "resize_before_merge": [["cntasm", "-k21", "-r", "-o", "@OUT@", "@A0@", "@A1@", "@A2@"]],
    "count_range_exclude_shrink": [["cntasm", "-k21", "-c1", "-x2", "-e1", "-s2", "-o", "@OUT@", "@A0@", "@A1@", "@A2@", "@A1@"]],
    "resume": [["cntasm", "-k21", "-o", "@OUT@", "@A0@", "@A1@"], ["cntasm", "-k21", "-i", "@OUT@", "-o", "@OUT@", "@A2@"]],
}
TABLE_CMDS = {
    "recount": [["recount", "-o", "@OUT@", "@digits@", "@half@"]],
    "subtract": [["subtract", "-o", "@OUT@", "@T0@", "@T1@"]],
    "isec2": [["isec", "-o", "@OUT@", "@T0@", "@T1@"]],
    "isec3": [["isec", "-o", "@OUT@", "@T0@", "@T1@", "@T2@"]],
}


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def entry(data):
    e = {"md5": hashlib.md5(data).hexdigest(), "bytes": len(data)}
    if len(data) <= TEXT_MAX:
        e["text"] = data.decode()
    return e


def expected(e, got):
    return hashlib.md5(got).hexdigest() == e["md5"] and len(got) == e["bytes"] and ("text" not in e or got.decode() == e["text"])


def digits_fa():
    """four 300-base sequences, written 1, 15, 150 and 1100 times: canonical 21-mers with counts 1, 15, 150 and 1023 (saturated)"""
    r = T.SplitMix64(SEED)
    rec = []
    for j, times in enumerate((1, 15, 150, 1100)):
        s = bytes(T.rand_seq(r, 300))
        rec += [(b"s%d_%d" % (j, i), s) for i in range(times)]
    return rec


def make_inputs(d):
    """write digits.fa, digits_half.fa, sparse.fq, asm0..2.fa and t0..2.yak into d; returns {name: path}"""
    rec = digits_fa()
    files = {"digits.fa": T.fasta(rec), "digits_half.fa": T.fasta(rec[::2])}
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, name)
        with open(paths[name], "wb") as f:
            f.write(data)
    paths["sparse.fq"] = os.path.join(d, "sparse.fq")
    subprocess.check_call([V.SYN, "-n", "300", "-l", "150", "-g", "40000", "-s", "31", "-o", paths["sparse.fq"]])
    for j, fa in enumerate(V.cntasm_assemblies(pathlib.Path(d))):
        paths["asm%d.fa" % j] = fa
    g = V.gold()
    sub = [pathlib.Path(d) / "setop", pathlib.Path(d) / "core"]
    for q in sub:
        q.mkdir()
    tabs = V.k25_tables(sub[0], V.SET_OP_READS, g["set_op_tables"]) + V.k25_tables(sub[1], V.CORE_READS, g["restore_core_tables"])[1:2]
    for j, t in enumerate(tabs):
        paths["t%d.yak" % j] = t
    return paths


def table_path(name, d):
    return os.path.join(d, name + ".yak") if name in MADE_TABLES else os.path.join(GOLD, name + ".yak")


def make_tables(exe, d, p, extra=()):
    """the tables made for the purpose, counted by `exe count` (the reference, the oracle's CLI or yak-amd) into d"""
    for name, (args, src) in MADE_TABLES.items():
        subprocess.run([exe, "count"] + args + list(extra) + ["-o", table_path(name, d), p[src]], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)


def fill(args, d, p, out):
    """a case's command line with its placeholders replaced"""
    def one(a):
        if a == "@OUT@":
            return out
        if a == "@half@":
            return p["digits_half.fa"]
        if a[:2] == "@A":
            return p["asm%s.fa" % a[2]]
        if a[:2] == "@T":
            return p["t%s.yak" % a[2]]
        return table_path(a[1:-1], d) if a[:1] == "@" else a
    return [one(a) for a in args]


def run_case(exe, steps, d, p, out, to_stdout=False, timeout=600):
    """run a case's command lines with `exe`; returns the bytes of its output file (to_stdout: of the last command's stdout, its -o left out)"""
    data = b""
    for i, args in enumerate(steps):
        a = fill(args, d, p, out)
        last = to_stdout and i == len(steps) - 1
        if last:
            at = a.index("-o")
            del a[at:at + 2]
        r = subprocess.run([exe] + a, check=True, stdout=subprocess.PIPE if last else subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout)
        data = r.stdout
    return data if to_stdout else open(out, "rb").read()


def ref_print(yak, fn, counts):
    return subprocess.run([yak, "print"] + (["-c"] if counts else []) + [fn], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, timeout=600).stdout


def main():
    if not os.path.exists(REF_YAK):
        sys.exit("build the reference first: make -C oracle ref")
    out = {"seed": SEED, "inputs": {}, "tables": {}, "print": {}, "cntasm": {}, "table_cmds": {}}
    with tempfile.TemporaryDirectory() as d:
        p = make_inputs(d)
        out["inputs"] = {n: md5(f) for n, f in sorted(p.items())}
        make_tables(REF_YAK, d, p, ["-t1"])
        out["tables"] = {name: md5(table_path(name, d)) for name in MADE_TABLES}
        moved = []
        for name in PRINT_TABLES:
            fn = table_path(name, d)
            plain, cnt = ref_print(REF_YAK, fn, False), ref_print(REF_YAK, fn, True)
            k, pairs = U.file_order_pairs(fn)
            assert sorted(U.lines(pairs, k, True).splitlines()) == sorted(cnt.splitlines()), name
            changed = U.lines(pairs, k, True) != cnt               # yak_ch_tighten moved keys: the listing is not in the file's order
            if changed:
                moved.append(name)
            out["print"][name] = {"plain": entry(plain), "counts": entry(cnt), "tighten_changes_order": changed, "kmers": len(pairs)}
        assert moved, "no print case in which the listing differs from the file's order"
        # ... which a restore alone can cause (keys re-placed in file order).  That yak_ch_tighten itself moves keys is shown on the oracle:
        # its listing without the step must differ from the reference's for the table made for it
        from oracle import pyoracle
        assert U.oracle_print(pyoracle, table_path("sparse", d), True) == ref_print(REF_YAK, table_path("sparse", d), True)
        assert U.oracle_print(pyoracle, table_path("sparse", d), True, tighten=False) != ref_print(REF_YAK, table_path("sparse", d), True), \
            "yak_ch_tighten changes nothing in the sparse table: the tighten step would be untested"
        digits = sorted({len(str(c)) for _, c in U.file_order_pairs(table_path("digits", d))[1]})
        assert digits == [1, 2, 3, 4] and any(c == 1023 for _, c in U.file_order_pairs(table_path("digits", d))[1]), digits
        for name, steps in CNTASM.items():
            out["cntasm"][name] = entry(run_case(REF_YAK, steps, d, p, os.path.join(d, name + ".yak")))
            out["cntasm"][name].pop("text", None)
        want = V.gold()["cntasm"]
        for name in ("plain", "resize_before_merge"):              # the same two cases as tests/golden/ref_cli.json
            assert [out["cntasm"][name]["md5"], out["cntasm"][name]["bytes"]] == want[name], name
        for name, steps in TABLE_CMDS.items():
            out["table_cmds"][name] = entry(run_case(REF_YAK, steps, d, p, os.path.join(d, name + ".yak")))
            out["table_cmds"][name].pop("text", None)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes; tighten changes the order of", moved)


if __name__ == "__main__":
    main()
