"""The range rule of the commands that walk a table's stored keys (yak_amd/csrc/table_ranges.h) against the three loops it replaced and against
its own properties, over a few thousand random size vectors: tests/tools/table_ranges_check.cpp, built with the host compiler and its address
and undefined-behaviour sanitizers and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_range_rule_equals_the_three_loops_it_replaced(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "table_ranges_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "tools", "table_ranges_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
