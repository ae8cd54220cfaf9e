"""Writes tests/golden/ref_cli.json: what the reference binary and library (oracle/_ref/yak, oracle/_ref/libyakref.so; built by
`make -C oracle ref` where the reference sources are) produce on the seeded inputs of tests/test_oracle_vs_ref.py and tests/test_qv.py.
Only data is stored: md5 and size of every .yak, digests of the qv output, the histograms `yak qv` printed.

    python tests/gen_golden_ref.py
"""
import ctypes as C
import json
import os
import pathlib
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_oracle_vs_ref as V          # noqa: E402
import test_qv as Q                     # noqa: E402
from conftest import GOLD, ROOT         # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "yak")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libyakref.so")


def ref(*args, stdout=None):
    return subprocess.run([REF] + list(args), check=True, stdout=stdout, stderr=subprocess.DEVNULL).stdout


def fresh(root, name):
    d = pathlib.Path(root) / name
    d.mkdir()
    return d


def main():
    if not os.path.exists(REF) or not os.path.exists(REF_LIB):
        raise SystemExit("oracle/_ref/ is not built: make -C oracle ref")
    out = {"produced_by": "the reference (oracle/_ref/yak, oracle/_ref/libyakref.so), tests/gen_golden_ref.py"}
    with tempfile.TemporaryDirectory() as tmp:
        d = fresh(tmp, "count")
        fq = V.cli_reads(d)
        out["count"] = {}
        for args in V.COMBOS:
            ref("count", *args, "-o", str(d / "a.yak"), fq)
            out["count"][V.combo_id(args)] = V.md5_size(str(d / "a.yak"))
        d = fresh(tmp, "two")
        ref("count", "-b24", "-o", str(d / "a.yak"), *V.two_input_reads(d))
        out["count_two_files"] = V.md5_size(str(d / "a.yak"))

        d = fresh(tmp, "cntasm")
        fas = V.cntasm_assemblies(d)
        out["cntasm"] = {}
        for pre_resize, name in ((0, "plain"), (1, "resize_before_merge")):
            ref("cntasm", "-k21", *(["-r"] if pre_resize else []), "-o", str(d / "a.yak"), *fas)
            out["cntasm"][name] = V.md5_size(str(d / "a.yak"))

        for key, specs in (("set_op_tables", V.SET_OP_READS), ("restore_core_tables", V.CORE_READS)):
            d = fresh(tmp, key)
            tabs = []
            for j, fq in enumerate(V.k25_reads(d, specs)):
                tabs.append(str(d / f"t{j}.yak"))
                ref("count", "-k25", "-o", tabs[-1], fq)
            out[key] = [V.md5_size(t) for t in tabs]
            if key == "set_op_tables":
                for cmd in ("subtract", "isec"):
                    ref(cmd, "-o", str(d / "a.yak"), *tabs)
                    out[cmd] = V.md5_size(str(d / "a.yak"))
            else:
                R = C.CDLL(REF_LIB)
                R.yak_ch_restore_core.restype = C.c_void_p
                R.yak_ch_dump.argtypes = [C.c_void_p, C.c_char_p]
                out["restore_core"] = {}
                for family in ("triobin", "sexchr"):
                    hr = None
                    for mode, fn in V.restore_core_steps(family, tabs):
                        hr = R.yak_ch_restore_core(C.c_void_p(hr), fn.encode(), C.c_int(mode), C.c_int(2), C.c_int(5))
                        assert hr
                    assert R.yak_ch_dump(C.c_void_p(hr), str(d / "a.yak").encode()) == 0
                    out["restore_core"][family] = V.md5_size(str(d / "a.yak"))

        from oracle import pyoracle
        d = fresh(tmp, "qv_cli")
        fq, fa = Q.qv_cli_inputs(d)
        ref("count", "-k27", "-b24", "-o", str(d / "t.yak"), fq)
        out["qv_cli"] = {"table": V.md5_size(str(d / "t.yak")), "output_md5": {}}
        for args in Q.QV_CLI_ARGS:
            text = ref("qv", *args, str(d / "t.yak"), fa, stdout=subprocess.PIPE).decode()
            out["qv_cli"]["output_md5"]["".join(args)] = Q.qv_digest(pyoracle.parse_qv_output(text))

        import hashlib
        out["qv_solve"] = {}
        for cov, e_asm in Q.QV_SOLVE_CASES:
            d = fresh(tmp, "qv_solve_" + Q.qv_solve_id(cov, e_asm))
            fq, fa = Q.qv_solve_inputs(d, cov, e_asm)
            ref("count", "-k21", "-b28", "-o", str(d / "t.yak"), fq)
            lines = ref("qv", str(d / "t.yak"), fa, stdout=subprocess.PIPE).decode().splitlines()
            ct = [l for l in lines if l.startswith("CT\t")]
            f = [l.split("\t") for l in ct]
            out["qv_solve"][Q.qv_solve_id(cov, e_asm)] = {
                "hist": {x[1]: int(x[2]) for x in f if int(x[2])}, "cnt": {x[1]: int(x[3]) for x in f if int(x[3])},
                "ct_md5": hashlib.md5("\n".join(ct).encode()).hexdigest(),
                "rest": [l for l in lines if l[:2] in ("FR", "ER", "CV", "QV")]}

        d = fresh(tmp, "qv_full")
        fq, fa = Q.qv_full_inputs(d)
        ref("count", "-k21", "-b28", "-o", str(d / "t.yak"), fq)
        lines = ref("qv", "-p", str(d / "t.yak"), fa, stdout=subprocess.PIPE).decode().splitlines()
        assert any(l.startswith("QV") for l in lines)
        out["qv_full"] = {"table": V.md5_size(str(d / "t.yak")), "output_md5": Q.qv_full_digest(lines)}
    with open(os.path.join(GOLD, "ref_cli.json"), "w") as fp:
        json.dump(out, fp, indent=1, sort_keys=True)
        fp.write("\n")


if __name__ == "__main__":
    main()
