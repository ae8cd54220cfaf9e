"""The host plan of the layout replay (yak_amd/csrc/replay_plan.h) against a put-by-put model of khashl's growth: tests/tools/replay_plan_check.cpp,
built with the host compiler and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replay_plan_keeps_khashl_growth_and_arena_invariants(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "replay_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "tools", "replay_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
