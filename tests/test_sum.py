"""The restatement of yakamd_ch_sum's result (tests/sum_util.py) against the CPU oracle alone: for unfiltered counts, the table of A plus the table
of B is the table of A ++ B.  No GPU; tests/test_gpu_sum.py holds the device to the same restatement."""
import ctypes as C

import numpy as np
import pytest

import sum_util as S


def o_count(oracle, img, k, pre=10):
    return oracle.lib().yko_count_mem(img, len(img), C.byref(oracle.copt(k=k, pre=pre)), None)


def o_bytes(oracle, o):
    try:
        return oracle.dump_bytes(o)
    finally:
        oracle.lib().yko_ch_destroy(o)


def o_merged(oracle, o0, o1, pre_resize):
    """the bytes of yko_ch_merge(o0, o1, 1, 1023, pre_resize); both tables are used up"""
    oracle.lib().yko_ch_merge(o0, o1, 1, 1023, pre_resize)          # frees o1 (htab.c:283)
    return o_bytes(oracle, o0)


@pytest.fixture(scope="module")
def images(synth):
    return S.operand_images(synth)


@pytest.mark.parametrize("pre_resize", [0, 1])
@pytest.mark.parametrize("k", [21, 31])
def test_sum_of_counts_is_the_count_of_the_concatenation(k, pre_resize, images, oracle):
    a, b = images
    ya, yb = o_bytes(oracle, o_count(oracle, a, k)), o_bytes(oracle, o_count(oracle, b, k))
    both = S.counts(o_bytes(oracle, o_count(oracle, a + b, k)))
    for x, y, ix, iy in ((ya, yb, a, b), (yb, ya, b, a)):             # unequal sizes, both orders
        merged = o_merged(oracle, o_count(oracle, ix, k), o_count(oracle, iy, k), pre_resize)
        exp = S.expected_sum_bytes(merged, x, y)
        assert S.counts(exp) == both
        assert len(exp) == len(merged) and S.parse(exp)[4].tolist() == S.parse(merged)[4].tolist()      # same sizes at the same places
    ca, cb = S.counts(ya), S.counts(yb)
    only_sum = [key for key, c in both.items() if c == 1023 and 0 < ca.get(key, 0) < 1023 and 0 < cb.get(key, 0) < 1023]
    assert len(only_sum) >= 30, "no k-mer passes 1023 in the sum alone"
    assert any(ca.get(key) == 1023 and 0 < cb.get(key, 0) < 1023 for key in both), "no k-mer at 1023 in the first table and present in the second"
    assert any(cb.get(key) == 1023 and key not in ca for key in both), "no k-mer at 1023 in the second table alone"
    assert any(0 < c < 1023 and ca.get(key, 0) and cb.get(key, 0) and c == ca[key] + cb[key] for key, c in both.items())


@pytest.mark.parametrize("k", [21, 31])
def test_keys_of_count_zero_contribute_nothing(k, images, oracle):
    """b = count(B), cleared, then B's first third counted into it: the other keys stay in b at count 0 and must not reach the sum"""
    O = oracle.lib()
    a, b = images
    part = b[:151 * 400]                                              # 400 whole reads
    ya = o_bytes(oracle, o_count(oracle, a, k))

    def make_b():
        o = o_count(oracle, b, k)
        O.yko_ch_clear(o)
        return O.yko_count_mem(part, len(part), C.byref(oracle.copt(k=k)), o)
    yb = o_bytes(oracle, make_b())
    cb = S.counts(yb)
    zeros = {key for key, c in cb.items() if c == 0}
    assert len(zeros) > 1000 and len(zeros) < len(cb)
    exp = S.expected_sum_bytes(o_merged(oracle, o_count(oracle, a, k), make_b(), 0), ya, yb)
    got = S.counts(exp)
    assert got == S.counts(o_bytes(oracle, o_count(oracle, a + part, k)))
    ca = S.counts(ya)
    assert not any(key in got for key in zeros if key not in ca) and any(key not in ca for key in zeros)


def test_a_changed_count_field_is_seen(images, oracle):
    """the comparisons above cannot pass vacuously: one count field off by one, and a key moved to a wrong count, are both seen"""
    a, b = images
    k = 21
    ya, yb = o_bytes(oracle, o_count(oracle, a, k)), o_bytes(oracle, o_count(oracle, b, k))
    exp = S.expected_sum_bytes(o_merged(oracle, o_count(oracle, a, k), o_count(oracle, b, k), 0), ya, yb)
    both = S.counts(o_bytes(oracle, o_count(oracle, a + b, k)))
    assert S.counts(exp) == both
    _, _, _, keys, heads = S.parse(exp)
    p = int(np.flatnonzero(np.diff(np.append(heads, len(exp))) > 8)[0])     # the first sub-table that holds a key
    at = int(heads[p]) + 8
    bad = bytearray(exp)
    bad[at] ^= 1                                                       # the lowest bit of the first key's count
    assert bytes(bad) != exp and S.counts(bytes(bad)) != both
    # ... and a merged image taken as it is (counts of the presence merge) is not the sum
    merged = o_merged(oracle, o_count(oracle, a, k), o_count(oracle, b, k), 0)
    assert merged != exp and S.counts(merged) != both and S.counts(merged).keys() == both.keys()
