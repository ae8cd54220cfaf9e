"""The invariant behind the count pass that raises every count in one sweep (engine_count.cpp yakamd_count_retained), stated
against the oracle alone, no GPU: in the filtered two-pass protocol (reference main.c:53-57, htab.c:62-74) the first pass counts every occurrence of
a k-mer but the first, which the filter takes, and the second pass counts every occurrence.  So after "pass 1, clear, pass 2 on the same reads" a
key's count c2 is min(c1 + 1, 1023), c1 its count after pass 1 -- except for the keys whose first occurrence the filter let through at once (a
false positive), which pass 1 counted in full already."""
import ctypes as C
import struct

import numpy as np
import pytest

SATURATION = b"A" * 2500 + b"\n" + b"T" * 900 + b"\n" + b"ACGTTGCA" * 300 + b"\n"     # tests/test_gpu_parity.py EDGE["saturation"]
# occurrence counts right at the cap: 1022 and 1024 of two k-mers each (period 2), 1023 of one
BOUNDARY = b"AG" * (15 + 1022) + b"\n" + b"C" * (30 + 1023) + b"\n" + b"AC" * (15 + 1024) + b"\n"


def table_counts(yak_bytes, pre=10):
    """{full hash: count} of a .yak image"""
    out, off = {}, 16
    for p in range(1 << pre):
        _, n = struct.unpack_from("<II", yak_bytes, off)
        off += 8
        e = np.frombuffer(yak_bytes, np.uint64, n, off)
        off += 8 * n
        out.update(zip(((e >> np.uint64(10)) << np.uint64(pre) | np.uint64(p)).tolist(), (e & np.uint64(1023)).tolist()))
    return out


def two_passes(oracle, img, k, bf_shift, pre=10, n_hash=4):
    """-> (c1, c2): the counts after pass 1 and after "destroy_bf, clear, pass 2 on the same reads" (no shrink)"""
    O = oracle.lib()
    oc = oracle.copt(k, pre, n_hash, bf_shift)
    o = O.yko_count_mem(img, len(img), C.byref(oc), None)
    try:
        c1 = table_counts(oracle.dump_bytes(o), pre)
        O.yko_ch_destroy_bf(o); O.yko_ch_clear(o)
        assert O.yko_count_mem(img, len(img), C.byref(oc), o)
        return c1, table_counts(oracle.dump_bytes(o), pre)
    finally:
        O.yko_ch_destroy(o)


def first_occurrence_false_positives(oracle, img, k, bf_shift, pre=10, n_hash=4):
    """-> ({hashes the oracle inserts on their FIRST occurrence}, {hash: occurrences}).  An occurrence after the first sets no bit its first one has not
    set (bbf.c:34-40), so the filter a first occurrence meets is the one the first occurrences before it made: a create pass over the first occurrences
    alone, in stream order, inserts exactly the keys whose first occurrence the filter lets through"""
    O = oracle.lib()
    f = O.yko_ch_init(k, pre, n_hash, bf_shift)
    occ = {}
    try:
        for a in oracle.extract_lists(k, pre, img):
            if not len(a):
                continue
            u, idx, cnt = np.unique(a, return_index=True, return_counts=True)
            occ.update(zip(u.tolist(), cnt.tolist()))
            firsts = np.ascontiguousarray(a[np.sort(idx)])
            O.yko_ch_insert_list(f, 1, len(firsts), firsts.ctypes.data_as(C.POINTER(C.c_uint64)))
        return set(table_counts(oracle.dump_bytes(f), pre)), occ
    finally:
        O.yko_ch_destroy(f)


CASES = {"reads_k31_b22": (lambda synth: synth(20000, g=90000, s=21), 31, 22), "reads_k21_b20": (lambda synth: synth(20000, g=90000, s=21), 21, 20),
         "saturation_k31_b20": (lambda synth: SATURATION, 31, 20), "boundary_k31_b20": (lambda synth: BOUNDARY, 31, 20)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_second_pass_count_is_first_pass_count_plus_one(case, oracle, synth):
    make, k, bf = CASES[case]
    img = make(synth)
    c1, c2 = two_passes(oracle, img, k, bf)
    fp, occ = first_occurrence_false_positives(oracle, img, k, bf)
    assert set(c1) == set(c2) and fp <= set(c1)
    odd = {x for x in c1 if c2[x] != min(c1[x] + 1, 1023)}
    assert odd <= fp, "%d keys off the rule that the filter did not let through on their first occurrence" % len(odd - fp)
    # what the rule rests on, key by key: pass 2 counts every occurrence, pass 1 all of them for a false positive and all but the first otherwise
    for x, n in occ.items():
        if x in c1:
            assert c2[x] == min(n, 1023) and c1[x] == min(n if x in fp else n - 1, 1023), (x, n, c1[x], c2[x])
        else:
            assert n == 1 and x not in fp
    if case.startswith("reads"):
        assert odd, "the input was chosen to have false positives: a filter of 2^%d bits" % bf
    if case.startswith("saturation"):
        assert max(occ.values()) > 1024 and max(c1.values()) == max(c2.values()) == 1023
    if case.startswith("boundary"):
        assert sorted(n for n in occ.values() if n >= 1022) == [1022, 1022, 1023, 1024, 1024]
        assert sorted(v for v in c1.values() if v >= 1021) == [1021, 1021, 1022, 1023, 1023]
        assert sorted(v for v in c2.values() if v >= 1021) == [1022, 1022, 1023, 1023, 1023]
