"""Writes tests/golden/adversarial.json: md5 and size of what the reference binary (oracle/_ref/yak, built by `make -C oracle ref` where the reference
sources are) counts on the images of tests/adversarial_util.py, `yak count -t1` with each option set of tests/test_adversarial.py.  Only those
figures are stored; the images are rebuilt from the builders.

    python tests/gen_golden_adversarial.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adversarial_util as A            # noqa: E402
import test_adversarial as T            # noqa: E402
from conftest import GOLD, ROOT         # noqa: E402
from gen_golden_ref import REF, ref     # noqa: E402


def fasta(path, img):
    with open(path, "wb") as fp:
        for i, rec in enumerate(img.split(b"\n")):
            if rec:
                fp.write(b">%d\n%s\n" % (i, rec))


def main():
    if not os.path.exists(REF):
        raise SystemExit("oracle/_ref/ is not built: make -C oracle ref")
    import conftest
    synth = conftest.synth.__wrapped__()            # the fixture's own function: the reads of tests/conftest.py
    out = {"produced_by": "the reference (oracle/_ref/yak count -t1), tests/gen_golden_adversarial.py", "count": {}}
    with tempfile.TemporaryDirectory() as tmp:
        fa, yak = os.path.join(tmp, "in.fa"), os.path.join(tmp, "out.yak")
        for name in T.NAMES + ["mixed"]:
            out["count"][name] = {}
            for oid, opt in T.OPTS.items():
                img = A.mixed(synth(**T.MIXED_SYNTH), opt["k"])["img"] if name == "mixed" else A.case(name, opt["k"])["img"]
                fasta(fa, img)
                ref("count", "-t1", "-k%d" % opt["k"], *(["-b%d" % opt["bf_shift"]] if "bf_shift" in opt else []), "-o", yak, fa)
                out["count"][name][oid] = T.md5_size(open(yak, "rb").read())
    with open(os.path.join(GOLD, "adversarial.json"), "w") as fp:
        json.dump(out, fp, indent=1, sort_keys=True)
        fp.write("\n")


if __name__ == "__main__":
    main()
