"""The tile arithmetic of the stable sort pass (yak_amd/csrc/seg_sort_tile.h, used by k_seg_sort_pass) on the CPU: tests/tools/seg_sort_check.cpp runs
whole multi-pass sorts through it, for the tile of either instantiation, segments of 0, 1, 2, tile - 1, tile, tile + 1 and 2 x tile + 1 keys and
uniform, one-valued and eight-valued digits, against std::stable_sort.  Built with the host compiler and its address and undefined-behaviour
sanitizers, run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_reorder_is_the_stable_sort_by_each_digit(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = str(tmp_path / "seg_sort_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "tools", "seg_sort_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
