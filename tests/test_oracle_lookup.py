"""The oracle's restatement of the lookup-only commands' per-position values (yko_lookup_image, qv.c:50-62 and
triobin.c:62-84) against the reference's own library: the same .yak loaded into oracle/_ref/libyakref.so, its
k-mers hashed with the reference's own hash functions (oracle/_ref/libyakshim.so) and encoded with its
seq_nt4_table, then looked up with its yak_ch_get.  tests/test_gpu_lookup.py relies on this restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libyakref.so")
REF_SHIM = os.path.join(ROOT, "oracle", "_ref", "libyakshim.so")

pytestmark = pytest.mark.skipif(not (os.path.exists(REF_LIB) and os.path.exists(REF_SHIM)), reason="reference library not built")


@pytest.fixture(scope="module")
def ref():
    R, S = C.CDLL(REF_LIB), C.CDLL(REF_SHIM)
    R.yak_ch_restore.restype = C.c_void_p; R.yak_ch_restore.argtypes = [C.c_char_p]
    R.yak_ch_restore_core.restype = C.c_void_p                     # variadic: (ch0, fn, mode, min_cnt, mid_cnt)
    R.yak_ch_get.restype = C.c_int; R.yak_ch_get.argtypes = [C.c_void_p, C.c_uint64]
    R.yak_ch_destroy.argtypes = [C.c_void_p]
    S.shim_hash64.restype = C.c_uint64; S.shim_hash64.argtypes = [C.c_uint64, C.c_uint64]
    S.shim_hash_long.restype = C.c_uint64; S.shim_hash_long.argtypes = [C.POINTER(C.c_uint64)]
    nt4 = bytes((C.c_ubyte * 256).in_dll(R, "seq_nt4_table"))
    return R, S, nt4


MOTIF = bytes(np.random.default_rng(0).choice(list(b"ACGT"), 200).tolist())     # counted 1100 times: its k-mers saturate at 1023


def query_image(synth, k):
    """~50 kb: reads of the counted genome with every kind of byte the encoders treat differently spliced in"""
    rng = np.random.default_rng(k)
    img = bytearray(synth(200, 150, 20000, s=3, e=0.01, N=0.002, first=50000) + synth(100, 150, 20000, s=4, e=0.01))
    odd = b"NnRYKMSWBDHVrykmswbdhv-.*\r\0\t @xX\x80\xff" + bytes([4, 5, 6, 7])
    for p in rng.integers(0, len(img), 400):
        img[p] = odd[rng.integers(0, len(odd))]
    for p in rng.integers(0, len(img), 3000):                         # lower case, U / u and raw codes 0-3: k-mer bases, not breaks
        img[p] = b"acgtUuUu\0\1\2\3"[rng.integers(0, 12)] if img[p] in b"ACGT" else img[p]
    run = bytes(rng.choice(list(b"AaCcGgTtUu\0\1\2\3"), 200).tolist())  # one window made of them alone
    return bytes(img) + run + b"\n" + MOTIF + b"\n"


def ref_walk(R, S, nt4, h, k, img, width):
    """triobin.c:62-84 / qv.c:50-62 in Python on the reference's own encoding, hashes and yak_ch_get"""
    nok = 0xFFFF if width == 2 else 0xFF
    out = np.full(len(img), nok, np.uint16 if width == 2 else np.uint8)
    mask = (1 << (2 * k if k < 32 else k)) - 1
    shift = 2 * (k - 1) if k < 32 else k - 1
    x, l = [0, 0, 0, 0], 0
    xl = (C.c_uint64 * 4)()
    for i, b in enumerate(img):
        c = nt4[b]
        if c >= 4:
            x, l = [0, 0, 0, 0], 0
            continue
        if k < 32:
            x[0] = (x[0] << 2 | c) & mask
            x[1] = x[1] >> 2 | (3 - c) << shift
        else:
            x[0] = (x[0] << 1 | (c & 1)) & mask
            x[1] = (x[1] << 1 | (c >> 1)) & mask
            x[2] = x[2] >> 1 | (1 - (c & 1)) << shift
            x[3] = x[3] >> 1 | (1 - (c >> 1)) << shift
        l += 1
        if l >= k:
            if k < 32:
                y = S.shim_hash64(min(x[0], x[1]), mask)
            else:
                xl[:] = x
                y = S.shim_hash_long(xl)
            out[i] = max(0, R.yak_ch_get(h, y))
    return out


def oracle_table(oracle, reads, k, pre, path):
    O = oracle.lib()
    h = O.yko_count_mem(reads, len(reads), C.byref(oracle.copt(k=k, pre=pre)), None)
    assert h and O.yko_ch_dump(h, path.encode()) == 0
    O.yko_ch_destroy(h)
    return path


def first_bad(got, want, img):
    bad = np.flatnonzero(got != want)
    return [(int(i), img[max(0, i - 3):i + 1], int(want[i]), int(got[i])) for i in bad[:5]]


@pytest.mark.parametrize("pre", [10, 14])
@pytest.mark.parametrize("k", [5, 21, 31, 32, 41, 63])
def test_lookup_image_equals_reference_get(k, pre, ref, oracle, synth, tmp_path):
    R, S, nt4 = ref
    O = oracle.lib()
    pat = oracle_table(oracle, synth(800, 150, 20000, s=3, e=0.01) + (MOTIF + b"\n") * 1100, k, pre, str(tmp_path / "pat.yak"))
    mat = oracle_table(oracle, synth(500, 150, 20000, s=3, e=0.01, first=9000) + synth(600, 150, 20000, s=4), k, pre, str(tmp_path / "mat.yak"))
    img = query_image(synth, k)
    # mode 1: the counts as stored (qv's u16 values; k >= 32 has no qv, the restatement still covers it)
    rh, oh = R.yak_ch_restore(pat.encode()), O.yko_ch_restore(pat.encode())
    assert rh and oh
    try:
        want = ref_walk(R, S, nt4, rh, k, img, 2)
        got = oracle.lookup_image(oh, img, 2)
        assert (got == want).all(), first_bad(got, want, img)
        assert (want == 0xFFFF).sum() > 0 and ((want == 0).sum() > 0 or k == 5) and (want > 1).sum() > 0 and (want == 1023).sum() > 0      # at k = 5 every k-mer is present
    finally:
        R.yak_ch_destroy(rh); O.yko_ch_destroy(oh)
    # modes 2 + 3: triobin's flags (u8)
    rh = R.yak_ch_restore_core(None, pat.encode(), 2, 2, 5)
    rh = R.yak_ch_restore_core(C.c_void_p(rh), mat.encode(), 3, 2, 5)
    oh = O.yko_ch_restore_core(None, pat.encode(), 2, 2, 5)
    oh = O.yko_ch_restore_core(oh, mat.encode(), 3, 2, 5)
    assert rh and oh
    try:
        want = ref_walk(R, S, nt4, rh, k, img, 1)
        got = oracle.lookup_image(oh, img, 1)
        assert (got == want).all(), first_bad(got, want, img)
        assert len(set(want[want <= 15].tolist())) >= 3 or k == 5
    finally:
        R.yak_ch_destroy(rh); O.yko_ch_destroy(oh)
