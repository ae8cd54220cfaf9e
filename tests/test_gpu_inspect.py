"""`yak inspect` on the device (k_inspect + yakamd_inspect / yakamd_inspect_tables): the joint spectrum against a numpy restatement and
the reference's own yak_ch_get, the reference binary's bytes under -R, resident and sharded tables, batching, and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import inspect_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "yak")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libyakref.so")
GENOME = 300000


def tiles(n, l, seed):
    L = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    L.yaksynth_tiles.restype = C.c_int64
    L.yaksynth_tiles.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int]
    buf = C.create_string_buffer(n * (l + 1))
    L.yaksynth_tiles(buf, n, l, seed, 4)
    return buf.raw


def fasta(fn, img):
    open(fn, "wb").write(b"".join(b">s%d\n%s\n" % (i, r) for i, r in enumerate(img.split(b"\n")) if r))
    return fn


@pytest.fixture(scope="module")
def tabs(tmp_path_factory, synth):
    """.yak files counted on the device: reads of genome 3 (unfiltered and -b20), an assembly of genome 3, reads of genome 9;
    per (k, pre); plus the FASTA inputs for yak_count()"""
    import yak_amd
    d = tmp_path_factory.mktemp("inspect")
    imgs = {"reads": synth(20000, 150, GENOME, 3), "asm": tiles(30, GENOME // 30, 3), "other": synth(8000, 150, 100000, 9)}
    made = {}

    def get(name, k, pre=10):
        key = (name, k, pre)
        if key not in made:
            src, bf = (name[:-3], 20) if name.endswith("_bf") else (name, 0)
            data, _ = yak_amd.count_protocol_host(imgs[src], k=k, pre=pre, bf_shift=bf)
            fn = str(d / ("%s_k%d_p%d.yak" % (name, k, pre)))
            open(fn, "wb").write(data)
            made[key] = fn
        return made[key]
    get.fa = {n: fasta(str(d / (n + ".fa")), img) for n, img in imgs.items()}
    get.dir = d
    return get


def run_cli(*args, check=True):
    r = subprocess.run([CLI, "inspect"] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if check:
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def restored(fn):
    import yak_amd
    h = yak_amd.lib().yak_ch_restore(fn.encode())
    assert h, yak_amd._err()
    return h


def device_joint(fa, fb, ref=False):
    import yak_amd
    L = yak_amd.lib()
    a = restored(fa)
    b = restored(fb) if fb else None
    try:
        return yak_amd.inspect_tables(a, b, ref)
    finally:
        L.yak_ch_destroy(a)
        if b:
            L.yak_ch_destroy(b)


def solver():
    import yak_amd
    return U.qv_solver(yak_amd.lib(), yak_amd.QstatT)


PAIRS = [(k, a, b) for k in (21, 31, 41, 63) for a, b in (("reads", "asm"), ("asm", "reads"), ("reads", "reads"), ("reads", "other"),
                                                             ("reads_bf", "asm"), ("reads", "reads_bf"))]
GOLDEN = [("nb_k27_p12.yak", "nb_k27_p12.yak"), ("b19_k31.yak", "b20_k31.yak"), ("nb_k31.yak", "nb_k31.yak"), ("nb_k41.yak", "nb_k41.yak"),
          ("nb_k21.yak", "nb_k21.yak"), ("b24_k63_fa.yak", "b24_k63_fa.yak")]


@pytest.mark.parametrize("k,a,b", PAIRS)
def test_joint_equals_numpy(tabs, k, a, b):
    fa, fb = tabs(a, k), tabs(b, k)
    A, B = U.read_yak(fa), U.read_yak(fb)
    for ref in (False, True):
        assert np.array_equal(device_joint(fa, fb, ref), U.joint(A, B, ref)), (k, a, b, ref)
    assert np.array_equal(device_joint(fa, None), U.joint(A))


@pytest.mark.parametrize("ga,gb", GOLDEN)
def test_joint_equals_numpy_golden(ga, gb):
    fa, fb = os.path.join(GOLD, ga), os.path.join(GOLD, gb)
    A, B = U.read_yak(fa), U.read_yak(fb)
    for ref in (False, True):
        assert np.array_equal(device_joint(fa, fb, ref), U.joint(A, B, ref)), (ga, gb, ref)


def test_pre12_against_pre10(tabs):
    """k < 32: the rebuilt hash is exact for any two pre"""
    fa, fb = tabs("reads", 27, 12), tabs("asm", 27, 10)
    A, B = U.read_yak(fa), U.read_yak(fb)
    for x, y, X, Y in ((fa, fb, A, B), (fb, fa, B, A)):
        J = device_joint(x, y)
        assert np.array_equal(J, U.joint(X, Y))
        assert J[:, 1:].sum() > 0


@pytest.mark.skipif(not os.path.exists(REFLIB), reason="reference library not built (make -C oracle ref)")
@pytest.mark.parametrize("k", [21, 31, 41, 63])
def test_sample_equals_reference_get(tabs, k):
    """c1 of a sample of keys through the reference's own yak_ch_restore + yak_ch_get(ch, (key >> 10) << pre | i)"""
    R = C.CDLL(REFLIB)
    R.yak_ch_restore.restype = C.c_void_p; R.yak_ch_restore.argtypes = [C.c_char_p]
    R.yak_ch_get.restype = C.c_int; R.yak_ch_get.argtypes = [C.c_void_p, C.c_uint64]
    R.yak_ch_destroy.argtypes = [C.c_void_p]
    fa, fb = tabs("reads", k), tabs("asm", k)
    A, B = U.read_yak(fa), U.read_yak(fb)
    ch = R.yak_ch_restore(fb.encode())
    assert ch
    try:
        idx = np.random.default_rng(k).choice(len(A[2]), 3000, replace=False)
        h = U.probe_hashes(A, False)[idx]
        want = np.array([max(0, R.yak_ch_get(ch, int(x))) for x in h], np.int64)
    finally:
        R.yak_ch_destroy(ch)
    J = device_joint(fa, fb)
    assert np.array_equal(U.Lookup(B).get(h), want)
    assert want.sum() > 0 and np.array_equal(J, U.joint(A, B))


@pytest.mark.parametrize("k", [21, 31, 41, 63])
def test_self_comparison_on_diagonal(tabs, k):
    fn = tabs("reads", k)
    J = device_joint(fn, fn)
    tot = J.sum(axis=1)
    assert np.array_equal(np.diag(J), tot) and J.sum() == len(U.read_yak(fn)[2])
    assert (J - np.diag(np.diag(J))).sum() == 0
    Jr = device_joint(fn, fn, ref=True)              # the reference's probe: most keys are not found in their own table
    assert np.trace(Jr) < tot.sum() // 2


@pytest.mark.skipif(not os.path.exists(REF), reason="reference binary not built (make -C oracle ref)")
@pytest.mark.parametrize("k,a,b", [(21, "reads", "asm"), (31, "reads", "reads_bf"), (41, "asm", "reads"), (63, "reads", "other")])
def test_cli_equals_reference_binary(tabs, k, a, b):
    fa, fb = tabs(a, k), tabs(b, k)
    for m in (0, 1, 20, 60):
        want = subprocess.run([REF, "inspect", "-m", str(m), fa, fb], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
        assert run_cli("-R", "-m", m, fa, fb).stdout == want, (k, a, b, m)
    want = subprocess.run([REF, "inspect", fa], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
    assert run_cli(fa).stdout == want


@pytest.mark.skipif(not os.path.exists(REF), reason="reference binary not built (make -C oracle ref)")
@pytest.mark.parametrize("ga,gb", GOLDEN[:3])
def test_cli_equals_reference_binary_golden(ga, gb):
    fa, fb = os.path.join(GOLD, ga), os.path.join(GOLD, gb)
    for m in (0, 1, 20, 60):
        want = subprocess.run([REF, "inspect", "-m", str(m), fa, fb], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600).stdout
        assert run_cli("-R", "-m", m, fa, fb).stdout == want, (ga, gb, m)


@pytest.mark.parametrize("k,a,b", [(21, "reads", "asm"), (31, "reads", "reads"), (41, "asm", "reads"), (63, "reads_bf", "other")])
def test_default_text_equals_restatement(tabs, k, a, b):
    import yak_amd
    fa, fb = tabs(a, k), tabs(b, k)
    A, B = U.read_yak(fa), U.read_yak(fb)
    J = U.joint(A, B)
    for m in (0, 1, 20, 60):
        want = U.lines(J, U.Lookup(B).hist, True, m, k, solver())
        assert run_cli("-m", m, fa, fb).stdout == want, (k, a, b, m)
        assert yak_amd.inspect(fa, fb, max_cnt=m) == want
    assert run_cli(fa).stdout == U.lines(U.joint(A), np.zeros(1024, np.int64), False, 20, k, solver())


def _count(fa, k, bf=0):
    import yak_amd
    L = yak_amd.lib()
    co = yak_amd.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k, co.bf_shift = k, bf
    h = L.yak_count(fa.encode(), C.byref(co), None)
    assert h, yak_amd._err()
    return h


@pytest.mark.parametrize("k", [31, 41])
def test_resident_tables_equal_file_route(tabs, knob, monkeypatch, k):
    """yakamd_inspect_tables on yak_count()'s tables == the join of their dumps; also when A, B or both are sharded over two ranks of one device"""
    import yak_amd
    L = yak_amd.lib()
    fa_in, fb_in = tabs.fa["reads"], tabs.fa["asm"]
    want = None
    for sa, sb in ((1, 1), (2, 1), (1, 2), (2, 2)):
        hs = []
        for fin, s in ((fa_in, sa), (fb_in, sb)):
            if s == 2:
                monkeypatch.setenv("YAKAMD_GPUS", "2"); monkeypatch.setenv("YAKAMD_GPU_LIST", "0,0")
            else:
                monkeypatch.delenv("YAKAMD_GPUS", raising=False); monkeypatch.delenv("YAKAMD_GPU_LIST", raising=False)
            hs.append(_count(fin, k))
            assert L.yakamd_last_sweeps() == s
        try:
            J = yak_amd.inspect_tables(hs[0], hs[1])
            J1 = yak_amd.inspect_tables(hs[0], None)
            if want is None:
                fa, fb = str(tabs.dir / ("res_a%d.yak" % k)), str(tabs.dir / ("res_b%d.yak" % k))
                assert L.yak_ch_dump(hs[0], fa.encode()) == 0 and L.yak_ch_dump(hs[1], fb.encode()) == 0
                want = U.joint(U.read_yak(fa), U.read_yak(fb))
                assert np.array_equal(device_joint(fa, fb), want)
                want1 = U.joint(U.read_yak(fa))
            assert np.array_equal(J, want), (sa, sb)
            assert np.array_equal(J1, want1), (sa, sb)
        finally:
            for h in hs:
                L.yak_ch_destroy(h)


@pytest.mark.parametrize("k", [21, 63])
def test_batches_give_the_same_bytes(tabs, k):
    import yak_amd
    fa, fb = tabs("reads", k), tabs("asm", k)
    for two in (fb, None):
        want = yak_amd.inspect(fa, two)
        for bk in (7, 1000, 50000):                  # batches that split sub-tables; batches of many sub-tables
            assert yak_amd.inspect(fa, two, batch_keys=bk) == want, (two, bk)
        assert run_cli("-B", 7, fa, *([two] if two else [])).stdout == want


def _refused(tmp_path, fa, fb, what, **kw):
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


def test_refusals(tabs, tmp_path):
    import yak_amd
    L = yak_amd.lib()
    a21, a31, a41 = tabs("reads", 21), tabs("reads", 31), tabs("reads", 41)
    _refused(tmp_path, a31, a21, "different k")
    _refused(tmp_path, a41, tabs("asm", 41, 11), "same pre")
    _refused(tmp_path, a31, a31, "outside [0, 1023]", max_cnt=1024)
    bad = str(tmp_path / "bad.yak")
    open(bad, "wb").write(b"YAK\x01" + open(a31, "rb").read()[4:])
    _refused(tmp_path, bad, None, "wrong file magic")
    _refused(tmp_path, a31, bad, "wrong file magic")
    data = open(a31, "rb").read()
    cut = str(tmp_path / "cut.yak")
    open(cut, "wb").write(data[:len(data) - 12])
    _refused(tmp_path, cut, a31, "truncated")
    _refused(tmp_path, cut, None, "truncated")
    r = run_cli("-m", 1024, a31, check=False)
    assert r.returncode != 0 and r.stdout == b""
    # an open pass on B (and on A) is refused
    t = yak_amd.Table(31, 10, 4, 0)
    a = restored(a31)
    try:
        assert L.yakamd_pass_begin(t.h, 1) == 0
        J = np.zeros(1024 * 1024, np.int64)
        assert L.yakamd_inspect_tables(a, t.h, 0, J.ctypes.data_as(C.POINTER(C.c_int64))) == -1
        assert "open pass" in yak_amd._err()
        assert L.yakamd_inspect_tables(t.h, a, 0, J.ctypes.data_as(C.POINTER(C.c_int64))) == -1
        assert "open pass" in yak_amd._err()
        assert L.yakamd_inspect_dev(t.h, 31, 10, 0, 1, None, 0, None, 0, 0, None, None) == -1
        assert "open pass" in yak_amd._err()
        assert L.yakamd_pass_end(t.h) >= 0
    finally:
        t.close()
        L.yak_ch_destroy(a)
