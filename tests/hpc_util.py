"""Homopolymer compression restated twice, for tests/test_hpc.py and tests/test_gpu_hpc.py (include/yak_amd.h: position i of a base image is
dropped iff i > 0, i and i - 1 are both valid -- a code 0..3 under seq_nt4_table -- and hold the same code; a kept valid position is written as
'A' 'C' 'G' 'T', a kept invalid one as '\\n').  The first restatement is numpy on the image, the second itertools.groupby on one record's text."""
import itertools

import numpy as np

NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    NT4[ord(_c)] = NT4[ord(_c.lower())] = NT4[_i] = _i
NT4[ord("U")] = NT4[ord("u")] = 3


def keep_mask(img):
    code = NT4[np.frombuffer(img, np.uint8)]
    valid = code < 4
    keep = np.ones(len(code), bool)
    keep[1:] = ~(valid[1:] & valid[:-1] & (code[1:] == code[:-1]))
    return code, valid, keep


def compress(img):
    """the compressed image, without the fill"""
    code, valid, keep = keep_mask(img)
    out = np.where(valid, np.frombuffer(b"ACGT\n", np.uint8)[code], np.uint8(10))
    return out[keep].tobytes()


def padded(b):
    return b + b"\n" * (-len(b) % 16)


def remap(img, off, ln):
    """off_out, len_out of the sequences [off, off + ln) (ends clamped to the image)"""
    _, _, keep = keep_mask(img)
    cs = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    o = np.minimum(np.asarray(off, np.int64), len(img))
    e = np.minimum(o + np.asarray(ln, np.int64), len(img))
    return cs[o], (cs[e] - cs[o]).astype(np.uint32)


def pack(img):
    """the packed image of yakamd_feed_packed_dev: (code words, validity words) as uint32 arrays, positions behind the image zero"""
    code = NT4[np.frombuffer(img, np.uint8)]
    n = len(code)
    c = np.zeros((n + 31) // 32 * 32, np.uint64)
    v = np.zeros(len(c), np.uint64)
    c[:n] = code & 3
    c[:n][code >= 4] = 0
    v[:n] = code < 4
    codes = (c.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    valid = (v.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return codes[:(n + 15) // 16], valid


_UP = bytes.maketrans(b"acgtuU\x00\x01\x02\x03", b"ACGTTTACGT")


def compress_seq(seq):
    """one record's sequence: upper case, U read as T, every run of A, C, G or T one letter, any other byte left alone"""
    s = seq.translate(_UP)
    groups = itertools.groupby(enumerate(s), key=lambda t: t[1] if t[1] in b"ACGT" else -1 - t[0])
    return bytes(next(g)[1] for _, g in groups)


def compress_records(img):
    """the image of the host-compressed records of an image whose records each end in '\\n'"""
    return b"".join(compress_seq(r) + b"\n" for r in img.split(b"\n")[:-1])


def as_image(text):
    """a compressed record text as the device writes it: every byte that is not A, C, G or T becomes '\\n'"""
    a = np.frombuffer(text, np.uint8)
    return np.where(np.isin(a, np.frombuffer(b"ACGT", np.uint8)), a, np.uint8(10)).tobytes()


def random_image(n, seed, p_repeat=0.5, p_n=0.01, p_lower=0.2, p_nl=0.004):
    """n bytes: a base repeats its predecessor with probability p_repeat; N, lower case and record ends mixed in"""
    r = np.random.default_rng(seed)
    fresh = r.integers(0, 4, n)
    rep = r.random(n) < p_repeat
    idx = np.arange(n)
    src = np.where(~rep | (idx == 0), idx, 0)
    np.maximum.accumulate(src, out=src)                          # a repeated position takes the base of the last fresh one before it
    code = fresh[src]
    a = np.frombuffer(b"ACGT", np.uint8)[code].copy()
    low = r.random(n) < p_lower
    a[low] |= 0x20
    a[r.random(n) < p_n] = ord("N")
    a[r.random(n) < p_nl] = 10
    return a.tobytes()


# planted images: single letters, case and U, raw codes, runs of N, empty records, an image that ends without '\n', runs around 16 positions
PLANTED = [
    b"", b"A", b"\n", b"N", b"AAAAAAA\n", b"AANAA\n", b"Aa\n", b"TU\n", b"tuTU\n", b"ACGT\n", b"AAACCCGTTNNAAT\n",
    b"NNNNNN\n", b"\n\n\n", b"A\n\nA\n", b"AAAA", b"ACGTTTT", bytes([0, 0, 1, 1, 2, 3, 3, 10]), b"A\x00a\x01C\n", b"AAAA\nAAAA\n",
    b"A" * 70001 + b"C\n", b"G" * 15 + b"\n", b"G" * 16 + b"\n", b"G" * 17 + b"\n", b"XYZ..--\n", b"AAnnAA\n",
]


def plant_runs(img, every, l=150, seed=9):
    """homopolymer runs of up to 40 bases written over a share of the reads of a synthetic read set (reads of l bases, each followed by '\\n')"""
    a = np.frombuffer(img, np.uint8).copy()
    r = np.random.default_rng(seed)
    n = len(a) // (l + 1)
    for j in range(0, n, every):
        for _ in range(int(r.integers(1, 4))):
            m = int(r.integers(2, 41))
            p = int(r.integers(0, l - m + 1))
            a[j * (l + 1) + p:j * (l + 1) + p + m] = b"ACGT"[int(r.integers(0, 4))]
    return a.tobytes()
