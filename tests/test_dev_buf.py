"""The owners of device-pool memory (yak_amd/csrc/dev_buf.h: DevBuf, DevVec) over a pool made of malloc: tests/tools/dev_buf_check.cpp, built with
the host compiler and its address and undefined-behaviour sanitizers and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_free_once_and_a_failed_reserve_leaves_no_capacity(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "dev_buf_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "tools", "dev_buf_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
