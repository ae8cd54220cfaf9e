"""The exchange plan of a multi-GPU round (yak_amd/csrc/round_plan.h) against the four loops of yak_multi.cpp it replaced and against what a grouped
send / recv requires of it, over a few thousand random rounds: tests/tools/round_plan_check.cpp, built with the host compiler and its address and
undefined-behaviour sanitizers and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_round_plan_equals_the_four_loops_it_replaced(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "round_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "tools", "round_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
