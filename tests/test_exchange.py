"""The reference side of tests/test_gpu_exchange.py, checked without a GPU: the oracle's flat extraction (yko_extract_pos, k up to 63) against
yko_extract -- the per-prefix lists the counting driver itself builds, pinned to the reference through the count goldens --, the helpers of
tests/exchange_util.py against each other on records written by hand, the expected packed image against the host packer, and the properties
the shared images are built for."""
import numpy as np
import pytest

import exchange_util as xu


@pytest.fixture(scope="module")
def images(synth):
    return dict(all_bytes=xu.all_bytes_image(), random_3wg=xu.random_3wg_image(synth), low_complexity=xu.low_complexity_image(synth))


@pytest.mark.parametrize("k", [31, 32, 33, 63])
@pytest.mark.parametrize("name", ["all_bytes", "random_3wg", "low_complexity"])
def test_flat_extraction_lists_what_the_counting_driver_lists(name, k, oracle, images):
    """for every prefix, the flat hashes with that prefix, in stream order, are yko_extract's list of that prefix; the positions are the indices
    of the k-mers' last bases: strictly ascending, and exactly the positions that end a window of k bases under yko_nt4"""
    img = images[name]
    h, t = oracle.extract_pos(k, img)
    ok = oracle.nt4()[np.frombuffer(img, np.uint8)] < 4
    run = np.arange(1, len(img) + 1) - np.maximum.accumulate(np.where(ok, 0, np.arange(1, len(img) + 1)))   # bases since the last non-base
    assert np.array_equal(t, np.flatnonzero(run >= k).astype(np.uint32))
    for pre in (10, 3):
        lists = oracle.extract_lists(k, pre, img)
        p = (h & np.uint64((1 << pre) - 1)).astype(np.int64)
        assert sum(len(x) for x in lists) == len(h) > 0
        order = np.argsort(p, kind="stable")
        assert np.array_equal(h[order], np.concatenate(lists))
        assert np.array_equal(np.bincount(p, minlength=1 << pre), [len(x) for x in lists])


def test_flat_extraction_below_32_is_unchanged(oracle):
    """the k < 32 half of yko_extract_pos on a known answer: count.c:28-43 by hand"""
    L = oracle.lib()
    h, t = oracle.extract_pos(3, b"ACGTNAC\nGGG")
    m = (1 << 6) - 1
    # ACG: fw 0b000110, rv (CGT) 0b011011 -> fw; CGT: fw 0b011011, rv (ACG) 0b000110 -> rv; GGG: fw 0b101010, rv (CCC) 0b010101 -> rv
    assert t.tolist() == [2, 3, 10]
    assert h.tolist() == [L.yko_hash64(0b000110, m), L.yko_hash64(0b000110, m), L.yko_hash64(0b010101, m)]
    h, t = oracle.extract_pos(31, b"")
    assert len(h) == 0 and len(t) == 0


class _Flat:
    """stands in for the oracle: hands expect_tagged a flat extraction written by hand"""

    def __init__(self, h, t):
        self.h, self.t = np.array(h, np.uint64), np.array(t, np.uint32)

    def extract_pos(self, k, img):
        return self.h, self.t


def test_tagged_helpers_agree_on_hand_made_records():
    """pre = 3.  Prefix 1: rounds 0, 2 (two records) and 64 (the next workgroup).  Prefix 5: round 1 alone.  Prefix 6: rounds 0 and 1.  The tagged
    records below are written by hand, toggles included: prefix 1 starts at 0, prefix 6 at 1, and the records of a round stand in any order"""
    pre = 3

    def H(x, p):
        return x << pre | p
    flat = [(H(7, 1), 5), (H(9, 6), 1023), (H(3, 5), 1024), (H(9, 6), 1030), (H(7, 1), 2048), (H(8, 1), 2050), (H(2, 1), 65536 + 1)]
    ora = _Flat([h for h, _ in flat], [t for _, t in flat])

    def rec(x, tg, pos):
        return x << 12 | tg << 10 | pos
    rec8 = [rec(7, 0, 5), rec(8, 1, 2), rec(7, 1, 0), rec(2, 0, 1),       # prefix 1: [0, 1), [1, 3) with its round's two records swapped, [3, 4)
            rec(3, 0, 0),                                                  # prefix 5
            rec(9, 1, 1023), rec(9, 0, 6)]                                 # prefix 6
    bstart = [0, 0, 4, 4, 4, 4, 5, 7, 7]
    want, wb = xu.expect_tagged(ora, b"", 0, pre)
    assert wb.tolist() == bstart
    got = xu.decode_tagged(rec8, bstart)
    assert got.same_runs(want) and xu.toggles_alternate(got)
    assert want.of(1) == [(0, frozenset({(7, 5)})), (2, frozenset({(7, 0), (8, 2)})), (64, frozenset({(2, 1)}))]
    assert got.of(1) == [(0, frozenset({(7, 5)})), (1, frozenset({(7, 0), (8, 2)})), (0, frozenset({(2, 1)}))]
    assert got.of(6) == [(1, frozenset({(9, 1023)})), (0, frozenset({(9, 6)}))] and got.of(0) == [] and want.of(5) == [(1, frozenset({(3, 0)}))]
    assert xu.max_per_round(want) == 2 and xu.crosses_workgroups(want)
    assert not xu.crosses_workgroups(xu.expect_tagged(_Flat([h for h, _ in flat[:6]], [t for _, t in flat[:6]]), b"", 0, pre)[0])
    # what must not pass: a toggle that did not flip, a position in the round off by one, a record in the neighbouring round's run
    for bad in ([rec(7, 0, 5), rec(8, 0, 2), rec(7, 0, 0), rec(2, 0, 1)], [rec(7, 0, 5), rec(8, 1, 3), rec(7, 1, 0), rec(2, 0, 1)],
                [rec(7, 0, 5), rec(8, 0, 2), rec(7, 1, 0), rec(2, 0, 1)]):
        assert not xu.decode_tagged(bad + rec8[4:], bstart).same_runs(want)
    # the plain groups of the same records
    h, t, b = xu.expect_groups(ora, b"", 0, pre)
    assert b.tolist() == bstart and t.tolist() == [5, 2048, 2050, 65537, 1024, 1023, 1030]
    assert [int(x) for x in xu.sort_groups(bstart, np.array([H(8, 1), H(2, 1), H(7, 1), H(7, 1), H(3, 5), H(9, 6), H(9, 6)], np.uint64),
                                           np.array([2050, 65537, 2048, 5, 1024, 1030, 1023], np.uint32))[1]] == t.tolist()


def test_expected_packed_image_is_the_host_packers(oracle, images):
    """every code word and validity word of all_bytes -- which holds every byte value -- and of lengths around a word: the host packer
    (yakamd_pack_bases_host: a table path and, where the CPU has it, a 32-byte-wide path) writes what yko_nt4 says, zero behind the last position"""
    import yak_amd
    img = images["all_bytes"]
    assert xu.isolated_values(img) == set(range(256))
    for T, s in xu.SPECIAL_AT.items():
        assert img[T - 2:T + 2] == s
    assert len(img) > xu.WG + 64 and len(img) % 16 != 0
    nt4 = oracle.nt4()
    assert nt4.tolist() == [{0: 0, 1: 1, 2: 2, 3: 3}.get(v, {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(chr(v).upper(), 4)) for v in range(256)]
    for n in [len(img), 65536, 4097, 4096, 65, 64, 63, 33, 32, 31, 17, 16, 15, 1]:
        codes, valid = xu.expect_packed(oracle, img[:n])
        hc, hv = xu.split_packed(yak_amd.pack_bases_host(img[:n]), n)
        assert np.array_equal(hc, codes) and np.array_equal(hv, valid), n
    # the words by hand: 'A' 'c' 'G' 'u' 'N' 2 '\n' 'T'
    codes, valid = xu.expect_packed(oracle, b"AcGuN\x02\nT")
    assert codes.tolist() == [0 | 1 << 2 | 2 << 4 | 3 << 6 | 2 << 10 | 3 << 14, 0] and valid.tolist() == [0b10101111]


def test_images_are_what_the_gpu_tests_need(oracle, images):
    """random_3wg: three workgroups, a read across each workgroup boundary with 63 bases on its left; low_complexity: more than 8 records of one
    prefix in one round at pre = 3 and pre = 10; random_3wg: a prefix whose consecutive contributing rounds lie in different workgroups"""
    r3 = images["random_3wg"]
    assert 2 * xu.WG + 4096 < len(r3) <= 150000 and len(r3) % 16 != 0
    for T in (xu.WG, 2 * xu.WG):
        assert set(r3[T - 64:T + 12]) <= set(b"ACGT")
    lc = images["low_complexity"]
    assert len(lc) <= 150000 and len(images["all_bytes"]) <= 150000
    for k, pre in ((31, 10), (30, 8), (21, 10), (27, 3), (1, 3)):
        assert xu.max_per_round(xu.expect_tagged(oracle, lc, k, pre)[0]) > (1000 if k > 1 else 8)
        assert xu.crosses_workgroups(xu.expect_tagged(oracle, r3, k, pre)[0])
    # other prefixes share the rounds of the long runs
    runs, _ = xu.expect_tagged(oracle, lc, 31, 10)
    big = np.flatnonzero(np.diff(runs.start) > 200)
    assert len(big) >= 8 and sum(np.sum(runs.key == runs.key[i]) > 50 for i in big) >= 5
