"""The stable radix passes (k_seg_sort_pass: kern_layout.inc) around the edges of their tile: shards of a few sub-tables fed with k-mers constructed to
hash into them, as test_gpu_parity.py::test_seg_sort_pass_of_long_segments does, YAKAMD_TSORT = 0, the shard's bytes against the oracle's.

The input is one k-mer per 32-byte record, so the insertion time of record i is 32 x i + 30: the first digit of T has eight values only (the skewed
case: every tile fills eight runs), the second is uniform, the third thin.  A sub-table's keys come out in khashl's layout, which depends on the
order the sort hands them over in: a pair out of place moves slots."""
import hashlib
import random
import struct

import numpy as np
import pytest

import paths_util
from adversarial_util import canonical_kmers, records

pytestmark = pytest.mark.gpu

K, PRE = 31, 10
TILE256, TILE1024 = 256 * 8, 1024 * 4          # seg_sort_tile.h: sst_tile


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


# slice_sort: sort_big = n_sel / (phi - plo) >= 30000 picks the instance; YAKAMD_TSORT = 0 keeps k_ts_rank out
RAN256 = paths_util.E([paths_util.SORT256], [paths_util.SORT1024, "k_ts_rank"], rank_refused="==0")
RAN1024 = paths_util.E([paths_util.SORT1024], [paths_util.SORT256, "k_ts_rank"], rank_refused="==0")


def _kmers(lo, sizes, seed=11):
    """records of one canonical k-mer each: sizes[j] distinct ones that hash into sub-table lo + j, shuffled"""
    rnd = random.Random(seed)
    recs = []
    for p, per in enumerate(sizes, lo):
        recs.append(records(canonical_kmers([h << PRE | p for h in rnd.sample(range(1 << (2 * K - PRE)), 3 * per + 16)], K, per), K))
    out = np.concatenate(recs)
    np.random.RandomState(seed).shuffle(out)
    return out.tobytes()


def _sizes(yak_bytes):
    out, off = [], 16
    for _ in range(1 << PRE):
        _, n = struct.unpack_from("<II", yak_bytes, off)
        out.append(n); off += 8 + 8 * n
    return out


def _shard_against_oracle(ya, oracle, knob, lo, sizes, entry, what):
    hi = lo + len(sizes)
    img = _kmers(lo, sizes)
    want, _ = oracle.count_protocol_mem(img, k=K)
    got_sizes = _sizes(want)
    assert got_sizes[lo:hi] == list(sizes) and sum(got_sizes) == sum(sizes)          # every k-mer landed where it was meant to, once
    off = 16 + sum(8 + 8 * n for n in got_sizes[:lo])
    want_range = want[off:off + sum(8 + 8 * n for n in sizes)]
    knob("YAKAMD_TSORT", 0)
    t = ya.Table(K, PRE, 4, 0)
    try:
        assert ya.lib().yakamd_set_shard(t.h, lo, hi) == 0
        with paths_util.tally(ya.lib()) as ran:
            t.count_pass_host(1, img)
        md5, n = t.range_md5(lo, hi)
        assert (n, md5) == (len(want_range), hashlib.md5(want_range).hexdigest())
    finally:
        t.close()
    paths_util.hold(ran, entry, paths_util.names(ya.lib()), what)


def test_256_thread_tiles_at_their_edges(ya, oracle, knob):
    """one sub-table each of 1, 2, tile - 1, tile, tile + 1 and 2 x tile + 1 keys (tile = 2048): the early exits, a tile with its last lane idle, a
    full one, one key in a tile of its own, three tiles.  10 244 keys in six sub-tables: the 256-thread instance; T < 2^19, three passes"""
    T = TILE256
    _shard_against_oracle(ya, oracle, knob, 300, [1, 2, T - 1, T, T + 1, 2 * T + 1], RAN256, "256-thread tiles")


def test_1024_thread_tiles_at_their_edges(ya, oracle, knob):
    """a shard of two sub-tables with tile + 1 = 4097 and 60 000 keys: a mean of 32 048, so the 1024-thread instance sorts both -- one key in a tile of
    its own, and fifteen tiles the last of which is part full; T < 2^22, three passes"""
    _shard_against_oracle(ya, oracle, knob, 500, [TILE1024 + 1, 60000], RAN1024, "1024-thread tiles")


def test_three_digits_in_one_sub_table(ya, oracle, knob):
    """one sub-table of 70 000 keys (T = 32 x index + 30 < 2^22: the third digit has 35 values, the first eight): the later passes take their
    histograms from the first pass's sweep, and every pass must leave the order of the ones before it.  One sub-table of that size: the 1024-thread
    instance"""
    _shard_against_oracle(ya, oracle, knob, 777, [70000], RAN1024, "three digits")
