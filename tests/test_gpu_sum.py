"""yakamd_ch_sum / `yak-amd sum` on the device: the dumped bytes against the restatement of tests/sum_util.py on the oracle's merge (tests/test_sum.py
holds that restatement to the oracle's count of the concatenated input), a large unfiltered sum against a re-count, the second operand left alone,
sharded operands, refusals and the command line."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sum_util as S

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
T = 600


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1
    return yak_amd


def fasta(img, fn):
    with open(fn, "wb") as f:
        for i, r in enumerate(img.split(b"\n")[:-1]):
            f.write(b">r%d\n%s\n" % (i, r))
    return fn


@pytest.fixture(scope="module")
def inp(synth, tmp_path_factory):
    """the operands of tests/test_sum.py and a third one, as base images and as FASTA files"""
    d = tmp_path_factory.mktemp("sum")
    a, b = S.operand_images(synth)
    c = synth(800, g=20000, s=11, first=4200) + S.tandem(S.U3, 40)
    img = dict(a=a, b=b, c=c)
    return img, {n: fasta(x, str(d / (n + ".fa"))) for n, x in img.items()}


_oracle_yak = {}


def oracle_yak(oracle, fn, k, pre):
    """the oracle's .yak bytes of a file's unfiltered count, computed once"""
    key = (fn, k, pre)
    if key not in _oracle_yak:
        o = oracle.lib().yko_count_file(fn.encode(), C.byref(oracle.copt(k=k, pre=pre)), None)
        _oracle_yak[key] = oracle.dump_bytes(o)
        oracle.lib().yko_ch_destroy(o)
    return _oracle_yak[key]


def oracle_merged(oracle, fx, fy, k, pre, pre_resize):
    O = oracle.lib()
    o0, o1 = (O.yko_count_file(f.encode(), C.byref(oracle.copt(k=k, pre=pre)), None) for f in (fx, fy))
    O.yko_ch_merge(o0, o1, 1, 1023, pre_resize)                       # frees o1
    try:
        return oracle.dump_bytes(o0)
    finally:
        O.yko_ch_destroy(o0)


def lib_count(ya, fn, k, pre=10):
    L = ya.lib()
    o = ya.CoptT(); L.yak_copt_init(C.byref(o)); o.k, o.pre = k, pre
    h = L.yak_count(fn.encode(), C.byref(o), None)
    assert h, ya._err()
    return ya.Table(ptr=h)


def mem_count(ya, img, k, pre=10):
    t = ya.Table(k, pre, 4, 0)
    t.count_pass_host(1, img)
    return t


def n_keys(yak):
    return len(S.parse(yak)[3])


# ---- 1. bytes ----
@pytest.mark.parametrize("pre_resize", [0, 1])
@pytest.mark.parametrize("pre", [10, 12, 14])
@pytest.mark.parametrize("k", [21, 31, 41])
def test_sum_bytes_equal_the_restated_merge(k, pre, pre_resize, ya, oracle, inp):
    L = ya.lib()
    _, fa = inp
    for fx, fy in ((fa["a"], fa["b"]), (fa["b"], fa["a"])):            # unequal sizes, both orders
        t0, t1 = lib_count(ya, fx, k, pre), lib_count(ya, fy, k, pre)
        try:
            y0, y1 = t0.dump_bytes(), t1.dump_bytes()
            assert y0 == oracle_yak(oracle, fx, k, pre) and y1 == oracle_yak(oracle, fy, k, pre)
            assert L.yakamd_ch_sum(t0.h, t1.h, pre_resize) == 0, ya._err()
            want = S.expected_sum_bytes(oracle_merged(oracle, fx, fy, k, pre, pre_resize), y0, y1)
            got = t0.dump_bytes()
            assert got == want
            assert t0.tot == n_keys(got) > max(n_keys(y0), n_keys(y1))
            assert t1.dump_bytes() == y1
        finally:
            t0.close(); t1.close()


# ---- 2. saturation and keys of count 0 ----
def test_saturation_reaches_the_device_result(ya, oracle, inp):
    L, O = ya.lib(), oracle.lib()
    img, _ = inp
    k = 31
    t0, t1 = mem_count(ya, img["a"], k), mem_count(ya, img["b"], k)
    try:
        ca, cb = S.counts(t0.dump_bytes()), S.counts(t1.dump_bytes())
        assert L.yakamd_ch_sum(t0.h, t1.h, 0) == 0, ya._err()
        got = S.counts(t0.dump_bytes())
        o = O.yko_count_mem(img["a"] + img["b"], len(img["a"]) + len(img["b"]), C.byref(oracle.copt(k=k)), None)
        want = S.counts(oracle.dump_bytes(o))
        O.yko_ch_destroy(o)
        assert got == want
        assert sum(1 for key, c in got.items() if c == 1023 and 0 < ca.get(key, 0) < 1023 and 0 < cb.get(key, 0) < 1023) >= 30
        assert any(ca.get(key) == 1023 and 0 < cb.get(key, 0) < 1023 and got[key] == 1023 for key in got)
        assert any(cb.get(key) == 1023 and key not in ca and got[key] == 1023 for key in got)
    finally:
        t0.close(); t1.close()


@pytest.mark.parametrize("pre_resize", [0, 1])
def test_keys_of_count_zero_do_not_enter(pre_resize, ya, oracle, inp):
    L, O = ya.lib(), oracle.lib()
    img, _ = inp
    k = 21
    part = img["b"][:151 * 400]
    t0, t1 = mem_count(ya, img["a"], k), mem_count(ya, img["b"], k)
    o0 = O.yko_count_mem(img["a"], len(img["a"]), C.byref(oracle.copt(k=k)), None)
    o1 = O.yko_count_mem(img["b"], len(img["b"]), C.byref(oracle.copt(k=k)), None)
    try:
        t1.clear(); t1.count_pass_host(0, part)
        O.yko_ch_clear(o1); O.yko_count_mem(part, len(part), C.byref(oracle.copt(k=k)), o1)
        y0, y1 = t0.dump_bytes(), t1.dump_bytes()
        assert y0 == oracle.dump_bytes(o0) and y1 == oracle.dump_bytes(o1)
        c0, c1 = S.counts(y0), S.counts(y1)
        zeros = {key for key, c in c1.items() if c == 0 and key not in c0}
        assert len(zeros) > 1000
        assert L.yakamd_ch_sum(t0.h, t1.h, pre_resize) == 0, ya._err()
        O.yko_ch_merge(o0, o1, 1, 1023, pre_resize); o1 = None
        got = t0.dump_bytes()
        assert got == S.expected_sum_bytes(oracle.dump_bytes(o0), y0, y1)
        cg = S.counts(got)
        assert not (zeros & cg.keys()) and t0.tot == len(cg)
        assert all(cg[key] == c0.get(key, 0) + c for key, c in c1.items() if c and c0.get(key, 0) + c < 1023)
    finally:
        t0.close(); t1.close(); O.yko_ch_destroy(o0)
        if o1 is not None:
            O.yko_ch_destroy(o1)


# ---- 3. an unfiltered sum against a re-count, sub-tables growing many times ----
def test_large_unfiltered_sum_equals_the_recount(ya, synth):
    L = ya.lib()
    n = 1000000
    img = synth(n, s=3)
    cut = 151 * (n // 2 + 12345)                                       # unequal halves, cut between two reads
    t0, t1, tw = mem_count(ya, img[:cut], 31), mem_count(ya, img[cut:], 31), mem_count(ya, img, 31)
    try:
        assert t0.subtable(5)[0] >= 4096 and tw.tot > max(t0.tot, t1.tot) > 5000000
        assert L.yakamd_ch_sum(t0.h, t1.h, 0) == 0, ya._err()
        assert t0.tot == tw.tot
        J = ya.inspect_tables(t0, tw)                                  # J[c0][c1]: keys of the sum at count c0 whose count in the re-count is c1 (0: absent)
        assert J.sum() == tw.tot and np.trace(J) == tw.tot and J[0, 0] == 0
        assert J[2:, 2:].sum() > 1000000                              # ... most of them at counts a single half does not reach alone
    finally:
        t0.close(); t1.close(); tw.close()


# ---- 4. the second operand ----
def test_second_operand_is_untouched_and_no_host_mirror_is_built(ya, inp):
    L = ya.lib()
    img, _ = inp
    t0, t1 = mem_count(ya, img["a"], 31), mem_count(ya, img["b"], 31)
    try:
        before = t1.dump_md5()
        syncs = L.yakamd_host_syncs()
        assert L.yakamd_ch_sum(t0.h, t1.h, 1) == 0, ya._err()
        assert L.yakamd_host_syncs() == syncs
        assert t1.dump_md5() == before and t1.tot == n_keys(t1.dump_bytes())
        assert L.yakamd_ch_sum(t0.h, t1.h, 0) == 0                    # ... and can be added again
        assert t1.dump_md5() == before and L.yakamd_host_syncs() == syncs
    finally:
        t0.close(); t1.close()


# ---- 5. sharded operands ----
@pytest.fixture(scope="module")
def unsharded_sum(ya, inp):
    _, fa = inp
    t0, t1 = lib_count(ya, fa["a"], 23), lib_count(ya, fa["b"], 23)
    try:
        assert ya.lib().yakamd_ch_sum(t0.h, t1.h, 1) == 0, ya._err()
        return t0.dump_bytes(), t1.dump_bytes()
    finally:
        t0.close(); t1.close()


@pytest.mark.parametrize("which", ["first_sharded", "second_sharded", "both_sharded"])
def test_sharded_operands(which, ya, inp, unsharded_sum, monkeypatch):
    L = ya.lib()
    _, fa = inp
    ts = []
    try:
        for j, n in enumerate("ab"):
            if which == "both_sharded" or (which == "first_sharded") == (j == 0):
                monkeypatch.setenv("YAKAMD_GPUS", "2"); monkeypatch.setenv("YAKAMD_GPU_LIST", "0,0")
                ts.append(lib_count(ya, fa[n], 23))
                assert L.yakamd_last_sweeps() == 2
            else:
                monkeypatch.delenv("YAKAMD_GPUS", raising=False); monkeypatch.delenv("YAKAMD_GPU_LIST", raising=False)
                ts.append(lib_count(ya, fa[n], 23))
                assert L.yakamd_last_sweeps() == 1
        assert L.yakamd_ch_sum(ts[0].h, ts[1].h, 1) == 0, ya._err()
        got = ts[0].dump_bytes()
        assert got == unsharded_sum[0] and ts[0].tot == n_keys(got)
        assert ts[1].dump_bytes() == unsharded_sum[1]
    finally:
        for t in ts:
            t.close()


# ---- 6. three tables ----
def test_three_tables_in_sequence(ya, oracle, inp):
    L, O = ya.lib(), oracle.lib()
    img, _ = inp
    k = 21
    ts = [mem_count(ya, img[n], k) for n in "abc"]
    try:
        assert L.yakamd_ch_sum(ts[0].h, ts[1].h, 0) == 0 and L.yakamd_ch_sum(ts[0].h, ts[2].h, 1) == 0, ya._err()
        whole = img["a"] + img["b"] + img["c"]
        o = O.yko_count_mem(whole, len(whole), C.byref(oracle.copt(k=k)), None)
        want = S.counts(oracle.dump_bytes(o))
        O.yko_ch_destroy(o)
        assert S.counts(ts[0].dump_bytes()) == want and ts[0].tot == len(want)
    finally:
        for t in ts:
            t.close()


# ---- 7. refusals ----
def test_refusals_leave_the_first_table_alone(ya, inp):
    L = ya.lib()
    img, _ = inp
    small = img["c"]
    t0 = mem_count(ya, small, 21)
    others = dict(k=mem_count(ya, small, 23), pre=mem_count(ya, small, 21, 12), same=mem_count(ya, small, 21))
    fake = (C.c_uint64 * 16)()                                        # zeroed: no engine behind it
    fake_h = C.cast(fake, C.POINTER(ya.ChT))
    fake_h.contents.k, fake_h.contents.pre = 21, 10
    null = C.POINTER(ya.ChT)()
    try:
        md5 = t0.dump_md5()

        def refused(h0, h1, word):
            assert L.yakamd_ch_sum(h0, h1, 0) == -1
            assert word in ya._err(), ya._err()
            assert t0.dump_md5() == md5
        refused(t0.h, others["k"].h, "k 21 and 23")
        refused(t0.h, others["pre"].h, "pre 10 and 12")
        refused(t0.h, null, "not an engine table")
        refused(null, t0.h, "not an engine table")
        refused(t0.h, fake_h, "not an engine table")
        refused(fake_h, t0.h, "not an engine table")
        refused(t0.h, t0.h, "same")
        same = others["same"]
        for opened, h0, h1 in ((t0, t0.h, same.h), (same, t0.h, same.h)):       # an open pass on the first, then on the second operand
            assert L.yakamd_pass_begin(opened.h, 1) == 0
            try:
                assert L.yakamd_ch_sum(h0, h1, 0) == -1 and "open pass" in ya._err()
            finally:
                assert L.yakamd_pass_end(opened.h) == 0              # nothing was fed: no key added
            assert t0.dump_md5() == md5
        assert L.yakamd_ch_sum(t0.h, same.h, 0) == 0                   # the table still works
        assert t0.dump_md5() != md5 and t0.tot == same.tot
    finally:
        t0.close()
        for t in others.values():
            t.close()


# ---- yak_ch_merge itself on the accumulator path (pre > 13) into a non-empty table: its create pass adds the hits of existing keys to the delta array ----
@pytest.mark.parametrize("pre_resize", [0, 1])
def test_merge_into_a_nonempty_table_at_pre_14(pre_resize, ya, oracle, inp):
    L, O = ya.lib(), oracle.lib()
    _, fa = inp
    t0, t1 = lib_count(ya, fa["a"], 21, 14), lib_count(ya, fa["b"], 21, 14)
    o0, o1 = (O.yko_count_file(fa[n].encode(), C.byref(oracle.copt(k=21, pre=14)), None) for n in "ab")
    try:
        h1, t1.h = t1.h, None                                          # both merges free their second table
        L.yak_ch_merge(t0.h, h1, 2, 1023, 4, pre_resize)
        O.yko_ch_merge(o0, o1, 2, 1023, pre_resize)
        assert t0.dump_bytes() == oracle.dump_bytes(o0) and t0.tot == o0.contents.tot > 30000
    finally:
        t0.close(); O.yko_ch_destroy(o0)


def test_sum_tables_names_an_unreadable_file(ya, tmp_path):
    nope = str(tmp_path / "nope.yak")
    with pytest.raises(RuntimeError, match="cannot load .*nope.yak"):
        ya.sum_tables([nope, nope])


# ---- 8. the command line ----
def test_command_line(ya, oracle, inp, tmp_path):
    L, O = ya.lib(), oracle.lib()
    img, _ = inp
    fn = {}
    for n in "abc":
        t = mem_count(ya, img[n], 21)
        fn[n] = str(tmp_path / (n + ".yak"))
        assert L.yak_ch_dump(t.h, fn[n].encode()) == 0
        t.close()
    out = str(tmp_path / "out.yak")
    want = ya.sum_tables([fn["a"], fn["b"]])
    subprocess.run([CLI, "sum", "-o", out, fn["a"], fn["b"]], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    assert open(out, "rb").read() == want
    r = subprocess.run([CLI, "sum", fn["a"], fn["b"]], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    assert r.stdout == want
    o = O.yko_count_mem(img["a"] + img["b"], len(img["a"]) + len(img["b"]), C.byref(oracle.copt(k=21)), None)
    assert S.counts(want) == S.counts(oracle.dump_bytes(o))
    O.yko_ch_destroy(o)
    # -r, three tables, and the Python wrapper's `out`
    out3 = str(tmp_path / "out3.yak")
    subprocess.run([CLI, "sum", "-r", "-o", out3, fn["a"], fn["b"], fn["c"]], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    py3 = str(tmp_path / "py3.yak")
    assert ya.sum_tables([fn["a"], fn["b"], fn["c"]], out=py3, pre_resize=True) == py3
    assert open(out3, "rb").read() == open(py3, "rb").read() and hashlib.md5(open(out3, "rb").read()).digest() != hashlib.md5(want).digest()
    for args in (["sum"], ["sum", fn["a"]], ["sum", "-o", out]):
        u = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd sum") and u.stdout == b""
    bad = subprocess.run([CLI, "sum", fn["a"], str(tmp_path / "nope.yak")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    assert bad.returncode == 2 and bad.stdout == b"" and b"yak-amd sum" in bad.stderr
    top = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    lines = top.stderr.decode().splitlines()
    names = [l.split()[1] for l in lines if l.startswith("    yak-amd ")]
    assert top.returncode == 1 and names == "count qv triobin trioeval inspect chkerr sexchr print cntasm recount subtract isec version".split()
    at = lines.index("  beyond the reference:")
    assert at > max(i for i, l in enumerate(lines) if l.startswith("    yak-amd ")) and lines[at + 1].startswith("      yak-amd sum ")
