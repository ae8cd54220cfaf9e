"""The record formats between the extraction and the counting kernels (yak_amd/csrc/yk_device.h: RecFmt) on the host: "tagged records fit" against the
record's definition for every k in 1..63 and prefix in 0..16, the bytes of the four formats, and the layout of Chunk2 that the level-2 kernels read:
tests/tools/rec_fmt_check.cpp, built with the host compiler and its address and undefined-behaviour sanitizers and run as a program of its own.
The header includes the HIP runtime's, so those are on the include path; no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_record_formats_and_the_tagged_predicate(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers under " + rocm)
    exe = str(tmp_path / "rec_fmt_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "tools", "rec_fmt_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
