"""A table gives back every byte it took from the device pool: for each life cycle below, run twice, the pool's bytes in use after the table
is destroyed equal the bytes in use before it was created -- exactly, allocation sizes are deterministic.  The first run absorbs what the
process keeps for good (static flags, tally buffers, the stream cache).  Every life cycle that completes also checks the table's .yak bytes
against the oracle: a test that only frees proves little about what it freed.

The knob settings are those of the cases of the same name in tests/paths_util.py (test_gpu_parity.py).  On the 2000 reads of this test the
settings of "pass_in_two_slices" leave the pass in one slice (one batch holds the input), so "pass_in_slices" runs beside it: its settings cut
these reads into two slices.  "abandon_with_kept_batches" is the only way to hand kept batches to fast_abandon (a batch fed behind the kept
ones is counted as a slice instead): a feed before the kept one in stream order, with {hash, position} records."""
import ctypes as C
import tempfile

import pytest

import hpc_util as H
import paths_util

pytestmark = pytest.mark.gpu
DEV = 0


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def imgs(synth):
    return synth(2000, s=41), synth(2000, s=43, first=100000)


@pytest.fixture(scope="module")
def want(imgs, oracle):
    """the oracle's bytes, computed once per protocol"""
    a, b = imgs
    return {"b24": oracle.count_protocol_mem(a, k=31, bf_shift=24), "plain": oracle.count_protocol_mem(a, k=31),
            "b24_other": oracle.count_protocol_mem(a, k=31, bf_shift=24, buf2=b), "hpc": oracle.count_protocol_mem(H.compress(a), k=21)}


def in_use(L):
    """bytes of the pool handed out right now: the high-water mark, reset to the bytes in use, read again"""
    L.yakamd_peak_bytes(DEV, 1)
    return L.yakamd_peak_bytes(DEV, 0)


def on_device(L, buf):
    d = L.yakamd_dev_alloc(len(buf) + 64)              # (plain device memory, not the pool's)
    assert d and L.yakamd_memcpy_h2d(d, buf, len(buf)) == 0
    return d


def retained_protocol(ya, imgs, want, events):
    """create pass with a filter and retention on, then the count pass over the retained records"""
    L = ya.lib()
    d = on_device(L, imgs[0])
    t = ya.Table(31, 10, 4, 24)
    with paths_util.tally(L) as ran:
        assert L.yakamd_retain_input(t.h, 1) == 0
        t.count_pass(1, [(d, len(imgs[0]), 0)])
        assert L.yakamd_retained_instances(t.h) > 0
        t.destroy_bf(); t.clear()
        assert L.yakamd_pass_begin(t.h, 0) == 0
        assert L.yakamd_count_retained(t.h) == 0
        assert L.yakamd_pass_end(t.h) == 0 and L.yakamd_retained_instances(t.h) == 0
        t.shrink(2, 1023)
        assert (t.dump_bytes(), t.tot) == want["b24"]
    t.close()
    L.yakamd_dev_free(d)
    paths_util.hold(ran, paths_util.E(**events), paths_util.names(L))


def protocol_host(ya, imgs, want, bf, events):
    """the whole `yak count` protocol from host memory, with or without a filter"""
    with paths_util.tally(ya.lib()) as ran:
        for b in bf:
            assert ya.count_protocol_host(imgs[0], k=31, bf_shift=b) == want["b24" if b else "plain"]
    paths_util.hold(ran, paths_util.E(**events), paths_util.names(ya.lib()))


def abandon_with_kept(ya, imgs, want):
    """the second half of the stream is kept, then the first half arrives: the kept batch goes through the accumulator path"""
    L = ya.lib()
    a = imgs[0]
    cut = 151 * 1000
    d0, d1 = on_device(L, a[:cut]), on_device(L, a[cut:])
    t = ya.Table(31, 10, 4, 0)
    with paths_util.tally(L) as ran:
        t.count_pass(1, [(d1, len(a) - cut, cut), (d0, cut, 0)])
        assert (t.dump_bytes(), t.tot) == want["plain"]
    t.close()
    L.yakamd_dev_free(d0); L.yakamd_dev_free(d1)
    paths_util.hold(ran, paths_util.E(["k_acc_insert"], fast_abandoned=">0"), paths_util.names(L))


def count_other_input_shrink_tighten(ya, imgs, want, oracle):
    """a count-existing pass over another input (the pending counts), then shrink and tighten (a new arena each)"""
    L, O = ya.lib(), oracle.lib()
    t = ya.Table(31, 10, 4, 24)
    t.count_pass_host(1, imgs[0])
    t.destroy_bf(); t.clear()
    t.count_pass_host(0, imgs[1])
    t.shrink(2, 1023)
    assert (t.dump_bytes(), t.tot) == want["b24_other"]
    L.yak_ch_tighten(t.h)
    with tempfile.NamedTemporaryFile(suffix=".yak") as f:         # the oracle's table back from its bytes, tightened
        f.write(want["b24_other"][0]); f.flush()
        o = O.yko_ch_restore(f.name.encode())
    O.yko_ch_tighten(o)
    assert t.dump_bytes() == oracle.dump_bytes(o)
    t.close(); O.yko_ch_destroy(o)


def host_feed_hpc(ya, imgs, want):
    L = ya.lib()
    t = ya.Table(21, 10, 4, 0)
    assert L.yakamd_ch_set_hpc(t.h, 1) == 0
    t.count_pass_host(1, imgs[0])
    assert (t.dump_bytes(), t.tot) == want["hpc"]
    t.close()


def insert_lists(ya, oracle):
    L, O = ya.lib(), oracle.lib()
    t = ya.Table(31, 10, 4, 0)
    o = O.yko_ch_init(31, 10, 4, 0)
    for p, n in ((3, 300), (5, 9000), (3, 700)):                  # the second list outgrows the scratch buffer of the first
        a = [(O.yko_hash64(i * 2654435761 % (1 << 62), (1 << 62) - 1) >> 10 << 10) | p for i in range(n)]
        arr = (C.c_uint64 * n)(*a)
        assert L.yak_ch_insert_list(t.h, 1, n, arr) == O.yko_ch_insert_list(o, 1, n, arr)
    assert t.dump_bytes() == oracle.dump_bytes(o)
    t.close(); O.yko_ch_destroy(o)


def destroyed_in_open_pass(ya, imgs):
    L = ya.lib()
    d = on_device(L, imgs[0])
    t = ya.Table(31, 10, 4, 24)
    assert L.yakamd_pass_begin(t.h, 1) == 0
    assert L.yakamd_feed_bases_dev(t.h, d, len(imgs[0]), 0) == 0
    t.close()
    L.yakamd_dev_free(d)


CYCLES = {
    "subbucket_records": (dict(), lambda ya, imgs, want, oracle: retained_protocol(ya, imgs, want, dict(pass2_fused=">0"))),
    "prefix_records": (dict(YAKAMD_RETAIN2="0"), lambda ya, imgs, want, oracle: retained_protocol(ya, imgs, want, dict(pass2_prefix=">0"))),
    "general_path": (dict(YAKAMD_FAST="0"), lambda ya, imgs, want, oracle: protocol_host(ya, imgs, want, (0, 24), dict(ran=["k_acc_insert", "k_bf_set"], slices="==0"))),
    "budget_exceeded_midpass": (dict(YAKAMD_FAST_BUDGET="100000"), lambda ya, imgs, want, oracle: protocol_host(ya, imgs, want, (0, 24), dict(ran=["k_acc_insert"], fast_abandoned=">0"))),
    "abandon_with_kept_batches": (dict(YAKAMD_REC8="0"), lambda ya, imgs, want, oracle: abandon_with_kept(ya, imgs, want)),
    "pass_in_two_slices": (dict(YAKAMD_FAST_BUDGET="30000000", YAKAMD_BATCH="1048576"), lambda ya, imgs, want, oracle: protocol_host(ya, imgs, want, (0, 24), dict(fast_abandoned="==0"))),
    "pass_in_slices": (dict(YAKAMD_FAST_BUDGET="3000000", YAKAMD_BATCH="65536"), lambda ya, imgs, want, oracle: protocol_host(ya, imgs, want, (0, 24), dict(early_slices=">0", fast_abandoned="==0"))),
    "count_other_input_shrink_tighten": (dict(), lambda ya, imgs, want, oracle: count_other_input_shrink_tighten(ya, imgs, want, oracle)),
    "host_feed_hpc": (dict(), lambda ya, imgs, want, oracle: host_feed_hpc(ya, imgs, want)),
    "insert_list_scratch": (dict(), lambda ya, imgs, want, oracle: insert_lists(ya, oracle)),
    "destroyed_in_open_pass": (dict(), lambda ya, imgs, want, oracle: destroyed_in_open_pass(ya, imgs)),
}


@pytest.mark.parametrize("case", list(CYCLES))
def test_a_table_gives_back_every_byte(case, ya, imgs, want, oracle, knob):
    L = ya.lib()
    env, cycle = CYCLES[case]
    for k, v in env.items():
        knob(k, v)
    cycle(ya, imgs, want, oracle)                                 # what the process keeps for good is taken here
    before = in_use(L)
    cycle(ya, imgs, want, oracle)
    peak = L.yakamd_peak_bytes(DEV, 1)
    after = L.yakamd_peak_bytes(DEV, 0)
    print("%s: %d bytes in use before the table, %d at its peak, %d after it" % (case, before, peak, after))
    assert peak > before                                          # the reading does see the table's buffers
    assert after == before
