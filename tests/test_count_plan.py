"""The plan of a count into existing keys (yak_amd/csrc/count_plan.h) against the cascade of engine_pass.cpp it replaced -- count_own_plan,
count_lds_bytes, the conditions of count_by_ranges, their order, the refusal of the records that only the key-owning kernel reads -- over a few
thousand random tables and settings and hand cases at every limit: tests/tools/count_plan_check.cpp, built with the host compiler and its address
and undefined-behaviour sanitizers and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_count_plan_equals_the_cascade_it_replaced(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "count_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "tools", "count_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
