"""The host walk of `yak-amd unitigs` (yak_amd/csrc/unitig_walk.h) against the restatement of tests/graph_util.py: tests/tools/unitig_walk_check.cpp,
built with the host compiler -- once with the address and undefined-behaviour sanitizers, once with the thread sanitizer -- and run as a program of
its own on record files the restatement writes, at 1, 3 and 8 threads; its FASTA and its U line byte for byte, cycles and single nodes included.
No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

import graph_util as U
from test_graph import CASES, ROOT

SAN = {"asan": "-fsanitize=address,undefined", "tsan": "-fsanitize=thread"}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    d = tmp_path_factory.mktemp("walk")
    exe = {}
    for name, flag in SAN.items():
        exe[name] = str(d / ("unitig_walk_check_" + name))
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", flag, "-fno-sanitize-recover=all", "-pthread",
                        os.path.join(ROOT, "tests", "tools", "unitig_walk_check.cpp"), "-o", exe[name]], check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def record_files(oracle, synth, tmp_path_factory):
    """(file, FASTA, U line) per input: the hand cases, and reads with errors, enough of them for every thread to have a range of its own"""
    d = tmp_path_factory.mktemp("records")
    out = []
    inputs = [(n, k, U.image([r.encode() for r in recs]), 1) for n, (k, recs) in sorted(CASES.items())]
    inputs += [("reads_k31", 31, synth(2000, 150), 1), ("reads_k31_c3", 31, synth(2000, 150), 3), ("bubble_k31_c2", 31, U.image([r.encode() for r in CASES["bubble_k31"][1]]), 2)]
    for name, k, img, min_cnt in inputs:
        data, _ = oracle.count_protocol_mem(img, k=k, pre=10, bf_shift=0)
        fn = str(d / (name + ".yak"))
        open(fn, "wb").write(data)
        kk, x, c = U.members(fn)
        recs, st = U.graph(k, x, c, min_cnt)
        ug = U.unitigs(k, recs, min_cnt)
        rf = str(d / (name + ".rec"))
        U.record_file(rf, k, min_cnt, recs)
        out.append((name, rf, U.fasta_text(ug), U.u_line(ug).encode(), ug))
    return out


@pytest.mark.parametrize("san", sorted(SAN))
@pytest.mark.parametrize("threads", [1, 3, 8])
def test_walk_equals_restatement(programs, record_files, san, threads):
    kinds = set()
    for name, rf, fa, u_line, ug in record_files:
        for mode, want in (("fasta", fa), ("stats", u_line)):
            r = subprocess.run([programs[san], rf, str(threads), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0 and r.stderr == b"", (name, r.stderr.decode()[-2000:])
            assert r.stdout == want, (name, mode)
        kinds.update(("cycle" if u[3] else "single" if u[1] == 1 else "chain") for u in ug)
    assert kinds == {"cycle", "single", "chain"}


def test_walk_reports_broken_links(programs, tmp_path):
    """a link into a key that is no node, and two nodes that point at each other on sides that promise an end: a message, no walk without end"""
    N = U.NONE
    for recs in ([(0, 1 << 1 | 1, N, 5, 1), (1, N, N, 0, 0)], [(0, 1 << 1 | 0, N, 5, 1), (5, 0 << 1 | 0, 0 << 1 | 0, 5, 0x11)]):
        rf = str(tmp_path / "bad.rec")
        U.record_file(rf, 3, 1, recs)
        r = subprocess.run([programs["asan"], rf, "2", "fasta"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and b"walk: the links from key" in r.stderr
