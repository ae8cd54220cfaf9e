"""The sequential model of the correction kernels (tools/correct_model_check.cpp: the find, the trial image and the decisions with the very functions
of yak_amd/correct/correct_step.h, the texts of correct_text.h, the reader of correct_reader.h; built by tools/Makefile with the host compiler under
the address and undefined-behaviour sanitizers and run as a program of its own, nothing of it is loaded into Python) against the restatement of
tests/correct_util.py, byte for byte: the records, the tallies, the trial image and both texts in several chunk sizes -- on the hand-derived cases
of tests/test_correct.py, on tiny random tables and on the planted reads; its base codes against the oracle's table; and its refusals on a damaged
fix record."""
import gzip
import os
import random
import shutil
import subprocess

import pytest

import correct_util as K
from conftest import ROOT
from test_correct import CASES, G, HAND_TABLE, PLANTED, mut, random_case


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++") is not None and shutil.which("make") is not None, "no g++ or no make on the path: the model of the kernels cannot be built"
    d = str(tmp_path_factory.mktemp("correct_model")) + os.sep
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "correct_model_check", "O=" + d], check=True, capture_output=True, text=True)
    return d + "correct_model_check"


def run(program, table, reads, mode, *more):
    r = subprocess.run([program, table, reads, mode] + [str(m) for m in more], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout


def model_equals(program, tmp, name, reads, k, c, e, x, cx, chunks=(1 << 28, 1), records=None):
    """every output of the model against flat(); records: [(name, comment, quality)] per read, FASTA without"""
    records = records or [("r%d" % i, "", "") for i in range(len(reads))]
    tab, fn = str(tmp / (name + ".tab")), str(tmp / (name + ".fx"))
    K.model_file(tab, k, c, e, x, cx)
    with open(fn, "wb") as f:
        f.write(K.reads_text(records, reads))
    img, offs, lens = K.image([r.encode() for r in reads])
    d = K.flat(img, offs, lens, k, c, e, x, cx)
    want = ["%d %d %d %d %d %d %d %d %d" % tuple(int(r[f]) for f in ("at", "seq", "p", "st", "en", "from", "to", "fit", "why")) for r in d["recs"]]
    want += ["t " + " ".join(str(int(t[f])) for f in K.TALLY_FIELDS) for t in d["tal"]]
    assert run(program, tab, fn, "records").decode().splitlines() == want
    assert run(program, tab, fn, "trials") == d["trials"]
    out = [d["img"][int(o):int(o) + int(L)].decode() for o, L in zip(offs, lens)]
    for chunk in chunks:
        assert run(program, tab, fn, "report", chunk) == K.flat_report([r[0] for r in records], d, lens, k, c, e, True)
        assert run(program, tab, fn, "reads", chunk) == K.reads_text(records, out)
    return d, tab, fn


@pytest.fixture(scope="module")
def hand_table(tmp_path_factory):
    return K.oracle_table([s.encode() for s in HAND_TABLE], 5, tmp_path_factory.mktemp("correct") / "hand.yak")


def test_model_on_the_hand_cases(program, tmp_path, hand_table):
    for e in (1, 3):
        names = sorted(n for n in CASES if CASES[n][1] == e)
        recs = [(n, "a comment  of two" if i % 3 == 1 else "", "I" * len(CASES[n][0]) if i % 2 else "") for i, n in enumerate(names)]
        d = model_equals(program, tmp_path, "hand%d" % e, [CASES[n][0] for n in names], 5, 2, e, *hand_table, chunks=(1 << 28, 40, 1), records=recs)[0]
        assert [d["img"].split(b"\n")[i].decode() for i in range(len(names))] == [CASES[n][2] for n in names]


def test_model_reads_fasta_fastq_and_gzip(program, tmp_path, hand_table):
    """the same records as FASTA on several lines, as FASTQ with \\r\\n, gzipped: the normal form leaves, byte-equal for a read that needs no change"""
    tab = str(tmp_path / "h.tab")
    K.model_file(tab, 5, 2, 1, *hand_table)
    bad = mut(G, 12)
    texts = {"multi.fa": (">a  x y\n%s\n%s\n>b\n%s\n" % (bad[:11], bad[11:], G)).encode(),
             "crlf.fq": ("@a  x y\r\n%s\r\n+\r\n%s\r\n@b\r\n%s\r\n+b\r\n%s\r\n" % (bad, "I" * 30, G, "#" * 30)).encode()}
    texts["multi.fa.gz"] = gzip.compress(texts["multi.fa"])
    want_fa, want_fq = (">a  x y\n%s\n>b\n%s\n" % (G, G)).encode(), ("@a  x y\n%s\n+\n%s\n@b\n%s\n+\n%s\n" % (G, "I" * 30, G, "#" * 30)).encode()
    for name, text in texts.items():
        fn = tmp_path / name
        fn.write_bytes(text)
        assert run(program, tab, str(fn), "reads") == (want_fq if name.endswith(".fq") else want_fa)
        assert run(program, tab, str(fn), "report").decode().splitlines()[1:3] == ["S\ta\t30\t26\t5\t1\t1\t0\t0\t0", "X\ta\t12\tG\tC\t5"]


def test_model_on_tiny_random_tables(program, tmp_path):
    rng = random.Random(31)
    n_fixed = 0
    for it in range(30):
        k = (5, 9)[it % 2]
        src, reads = random_case(rng, k)
        x, cx = K.oracle_table([s.encode() for s in src], k, tmp_path / "t.yak")
        d = model_equals(program, tmp_path, "t%d" % it, reads, k, rng.choice((1, 2)) if len(src) > 3 else 1, rng.choice((1, 1, 2)), x, cx, chunks=(1 << 28, 1))[0]
        n_fixed += int((d["recs"]["why"] == K.DONE).sum())
    assert n_fixed > 10


def test_model_on_the_planted_reads(program, tmp_path):
    for k, seed in PLANTED:
        clean, bad = K.planted(k, seed)
        x, cx = K.oracle_table([r.encode() for r in clean], k, tmp_path / "p.yak", pre=12)
        d = model_equals(program, tmp_path, "p%d" % k, bad, k, 3, 1, x, cx, chunks=(1 << 28, 1000))[0]
        assert d["img"] == K.image([r.encode() for r in clean[::3]])[0]


def test_model_base_codes_are_the_tables(program):
    from oracle import pyoracle
    got = [int(v) for v in subprocess.run([program, "-", "-", "nt4"], check=True, stdout=subprocess.PIPE).stdout.split()]
    assert got == K.CODE.tolist() == pyoracle.nt4().tolist()


def test_model_refuses(program, tmp_path, hand_table):
    """a record whose base lies behind the image, whose run is longer than k, whose base is at neither place its run allows, or on a byte that is
    no base: a message, not a read outside"""
    d, tab, fn = model_equals(program, tmp_path, "ok", [mut(G, 12), G], 5, 2, 1, *hand_table)
    for what in ("damage-at", "damage-run", "damage-p", "damage-base"):
        r = subprocess.run([program, tab, fn, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and b"does not lie inside the image, or on a byte that is no base" in r.stderr, (what, r.stderr)
    r = subprocess.run([program, tab, str(tmp_path / "none.fa"), "report"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and b"cannot be opened" in r.stderr
