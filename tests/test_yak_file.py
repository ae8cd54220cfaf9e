"""The one reader of the .yak format (yak_amd/csrc/yak_file.h) against the three parsers it replaced -- restore's read_yak, parse_yak_image of the
unsharded copy, inspect's read_head and BodyReader -- on the golden tables, a few hundred random small images, one image cut at every byte offset
and the headers each caller refuses: tests/tools/yak_file_check.cpp, built with the host compiler and its address and undefined-behaviour
sanitizers and run as a program of its own.  No GPU, nothing loaded into Python."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_yak_reader_equals_the_three_parsers_it_replaced(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    golden = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.yak")))
    assert len(golden) >= 10
    exe = str(tmp_path / "yak_file_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "tools", "yak_file_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe] + golden, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
