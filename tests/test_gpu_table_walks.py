"""What the commands that walk a resident table's stored keys share (yak_amd/csrc/table_ranges.h, table_read.cpp): with a budget of one key, so
that every sub-table that holds keys is a range of its own and the empty ones fall between the ranges, hetmers, unitigs and print write what they
write in one range; and the calls that stage a range give every byte of it back to the device pool, refused or not."""
import ctypes as C

import numpy as np
import pytest

import hetmer_util as U

pytestmark = pytest.mark.gpu
DEV = 0


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def planted(ya, tmp_path_factory):
    """planted_k31_p10 of test_gpu_hetmers.py / test_gpu_graph.py: the table and the .yak file of its dump"""
    t = ya.Table(31, 10, 4, 0)
    t.count_pass_host(1, U.image(U.planted(31)))
    fn = str(tmp_path_factory.mktemp("walks") / "planted_k31_p10.yak")
    open(fn, "wb").write(t.dump_bytes())
    yield t, fn
    t.close()


def sizes(L, h, P):
    cap, size = C.c_uint32(), C.c_uint32()
    out = []
    for p in range(P):
        assert L.yakamd_subtable(h, p, C.byref(cap), C.byref(size)) == 0
        out.append(size.value)
    return out


def test_a_budget_of_one_key(ya, planted, knob, monkeypatch, capfd):
    """planted_k31_p10 holds 3871 keys in 1004 of its 1024 sub-tables, 1 to 14 each: sub-tables of one key, larger ones and empty ones between
    them.  Runs of empty sub-tables at both ends and budgets of every kind are tests/tools/table_ranges_check.cpp's"""
    t, fn = planted
    n = sizes(ya.lib(), t.h, 1024)
    holding = sum(1 for s in n if s)
    print("planted_k31_p10: %d keys in %d of 1024 sub-tables, of %d to %d keys" % (sum(n), holding, min(s for s in n if s), max(n)))
    assert 1 < holding < 1024 and max(n) > 1                      # empty sub-tables between the ranges, and ranges above the budget
    one = ya.hetmers(fn, pairs=True), ya.unitigs(fn), ya.print_table(t.h)
    assert one[0].count(b"\nK\t") == 28 and one[1].startswith(b">") and one[2].count(b"\n") == sum(n)
    knob("YAKAMD_HETMER_BATCH", 1)
    knob("YAKAMD_GRAPH_BATCH", 1)
    monkeypatch.setenv("YAKAMD_VERBOSE", "1")                     # the commands tell their ranges
    capfd.readouterr()
    got = ya.hetmers(fn, pairs=True), ya.unitigs(fn), ya.print_table(t.h, batch_bytes=1)
    said = capfd.readouterr().err
    assert got[0] == one[0]
    assert got[1] == one[1]
    assert got[2] == one[2]
    assert "hetmers: %d ranges of keys" % holding in said and "unitigs: %d ranges of records" % holding in said, said[-2000:]


def in_use(L):
    """bytes of the pool handed out right now (test_gpu_ctx_buffers.py): the high-water mark, reset to the bytes in use, read again"""
    L.yakamd_peak_bytes(DEV, 1)
    return L.yakamd_peak_bytes(DEV, 0)


def test_staged_ranges_go_back_to_the_pool(ya, planted):
    L = ya.lib()
    t, fn = planted
    even = ya.Table(30, 10, 4, 0)                                 # refused by the het-mer calls, of another k for inspect
    J = np.zeros(1024 * 1024, np.int64)
    Jp = J.ctypes.data_as(C.POINTER(C.c_int64))
    out = C.POINTER(C.c_uint8)()
    d = L.yakamd_dev_alloc(64)                                    # (plain device memory, not the pool's)

    n_keys = len(ya.kmers(t.h)[0])

    def inspect_one():
        assert L.yakamd_inspect_tables(t.h, None, 0, Jp) == 0 and int(J.sum()) == n_keys

    calls = {
        "yakamd_hetmers_dev": lambda: t.hetmers(1),
        "yakamd_hetmer_pairs_dev": lambda: t.hetmer_pairs(1),     # a size query, then the full call
        "yakamd_kmers_dev": lambda: ya.kmers(t.h),                # (likewise)
        "yakamd_inspect_tables": inspect_one,
        "yakamd_dump_range_mem": lambda: t.range_md5(0, 1024),
    }
    refused = {
        "yakamd_hetmers_dev": lambda: L.yakamd_hetmers_dev(even.h, 1, d, d, None),
        "yakamd_hetmer_pairs_dev": lambda: L.yakamd_hetmer_pairs_dev(even.h, 1, None, 0),
        "yakamd_kmers_dev": lambda: L.yakamd_kmers_dev(t.h, 0, 1025, None, None, 0),
        "yakamd_inspect_tables": lambda: L.yakamd_inspect_tables(t.h, even.h, 0, Jp),
        "yakamd_dump_range_mem": lambda: L.yakamd_dump_range_mem(t.h, 5, 5, C.byref(out)),
    }
    try:
        for name, call in calls.items():
            call()                                                # what the process keeps for good is taken here
            before = in_use(L)
            call()
            peak = L.yakamd_peak_bytes(DEV, 1)
            after = L.yakamd_peak_bytes(DEV, 0)
            print("%s: %d bytes in use before, %d at the peak, %d after" % (name, before, peak, after))
            assert peak > before, name                            # the reading does see the staged range
            assert after == before, name
            assert refused[name]() == -1, name
            assert in_use(L) == before, name + ", refused"
    finally:
        L.yakamd_dev_free(d)
        even.close()
