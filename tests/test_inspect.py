"""`yak inspect` on the device, host tier: the entry points are exported and declared, the options default as the reference's, and the
errors caught before any device call (usage, a wrong magic, a truncated header) -- and without a GPU the call fails instead of joining on the
CPU.  The numpy restatement the GPU tests use equals the reference binary where it is built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import inspect_util as U

CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "yak")
NEW = ["yakamd_inspect_dev", "yakamd_inopt_init", "yakamd_inspect", "yakamd_inspect_tables"]


def test_inspect_entry_points_exported_and_declared():
    import yak_amd
    L = yak_amd.lib()
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(yak_amd.YAK_AMD_H_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "yak_amd.h")).read()
    for n in NEW + ["yakamd_inopt_t"]:
        assert n in hdr, n


def test_inopt_defaults():
    import yak_amd
    o = yak_amd.InoptT()
    yak_amd.lib().yakamd_inopt_init(C.byref(o))
    assert (o.max_cnt, o.ref_probe, o.n_threads, o.batch_keys) == (20, 0, 4, 1 << 24)   # inspect.c:11
    assert C.sizeof(yak_amd.InoptT) == 24


def cli(*args):
    return subprocess.run([CLI, "inspect"] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_usage():
    for args in ((), ("a.yak", "b.yak", "c.yak"), ("-q", "a.yak")):
        r = cli(*args)
        assert r.returncode == 1 and r.stdout == b""
    assert b"inspect [options] <in1.yak> [in2.yak]" in cli().stderr
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"yak-amd inspect" in r.stderr


def _fails(tmp_path, fa, fb, what, **kw):
    import yak_amd
    L = yak_amd.lib()
    o = yak_amd.InoptT()
    L.yakamd_inopt_init(C.byref(o))
    for f, v in kw.items():
        setattr(o, f, v)
    out = str(tmp_path / "out.txt")
    assert L.yakamd_inspect(C.byref(o), fa.encode(), fb.encode() if fb else None, out.encode()) == -1
    assert what in yak_amd._err(), yak_amd._err()
    assert not os.path.exists(out)


def test_file_errors_before_the_device(tmp_path):
    good = os.path.join(GOLD, "nb_k31.yak")
    data = open(good, "rb").read()
    bad = str(tmp_path / "bad.yak")
    open(bad, "wb").write(b"KAY\x02" + data[4:])
    short = str(tmp_path / "short.yak")
    open(short, "wb").write(data[:10])
    bits = str(tmp_path / "bits.yak")
    open(bits, "wb").write(data[:12] + (8).to_bytes(4, "little") + data[16:])
    for fa, fb, what in ((bad, None, "wrong file magic"), (good, bad, "wrong file magic"), (short, None, "truncated header"),
                         (good, short, "truncated header"), (bits, None, "counter bits"), (str(tmp_path / "none.yak"), None, "cannot open"),
                         (good, os.path.join(GOLD, "nb_k21.yak"), "different k"), (os.path.join(GOLD, "nb_k41.yak"), None, "")):
        if what:
            _fails(tmp_path, fa, fb, what)
    _fails(tmp_path, good, None, "outside [0, 1023]", max_cnt=1024)
    _fails(tmp_path, good, good, "outside [0, 1023]", max_cnt=-1)
    r = cli(bad)
    assert r.returncode == 2 and r.stdout == b"" and b"wrong file magic" in r.stderr


def test_no_cpu_fallback_without_gpu(tmp_path):
    """without a gfx950 device inspect fails with a message; it never tallies the keys on the CPU"""
    import yak_amd
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    good = os.path.join(GOLD, "nb_k31.yak")
    _fails(tmp_path, good, None, "no gfx950")
    _fails(tmp_path, good, good, "no gfx950")
    r = cli(good)
    assert r.returncode == 2 and r.stdout == b""


@pytest.mark.skipif(not os.path.exists(REF), reason="reference binary not built (make -C oracle ref)")
def test_restatement_equals_reference_binary():
    """the numpy J of the reference's probe, printed as inspect.c prints it, is the reference binary's output; the reference finds 10 of
    nb_k31's 15169 keys in nb_k31 itself and 4 of b19's 2586 keys in b20, where the rebuilt hash finds all of them"""
    import yak_amd
    solve = U.qv_solver(yak_amd.lib(), yak_amd.QstatT)
    for ga, gb, found in (("nb_k31.yak", "nb_k31.yak", (10, 15169)), ("b19_k31.yak", "b20_k31.yak", (4, 2586))):
        fa, fb = os.path.join(GOLD, ga), os.path.join(GOLD, gb)
        A, B = U.read_yak(fa), U.read_yak(fb)
        J = U.joint(A, B, ref=True)
        assert (J[:, 1:].sum(), J.sum()) == found
        assert U.joint(A, B)[:, 1:].sum() == found[1]
        for m in (0, 20):
            want = subprocess.run([REF, "inspect", "-m", str(m), fa, fb], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60).stdout
            assert U.lines(J, U.Lookup(B).hist, True, m, A[0], solve) == want
        want = subprocess.run([REF, "inspect", fa], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60).stdout
        assert U.lines(U.joint(A), np.zeros(1024, np.int64), False, 20, A[0], solve) == want
