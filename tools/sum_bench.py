"""Time yakamd_ch_sum on the two halves of the benchmark's reads (bench.py: 10 M x 150 bp, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %), each counted
unfiltered at k = 31: one JSON line with the wall time of the sum, of yak_ch_merge(h0, h1, 0, 1023, ...) on the same operands and of re-counting
the concatenation (one pass, the halves fed one behind the other from page-locked host memory), and whether the sum equals the re-count
(yakamd_inspect_tables: every key on the diagonal).  --only sum stops after the sum: the run to put under `rocprofv3 --kernel-trace --stats`,
whose kernel table splits the sum into the create pass and k_img_add_counts.
Usage: python tools/sum_bench.py [--reads 10000000] [--only sum]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN, K = 150, 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--only", choices=["sum"], default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    half, genome = a.reads // 2, 5 * a.reads
    nb = half * (READ_LEN + 1)
    bufs = []
    for j in range(2):
        p = L.yakamd_host_alloc(nb)
        assert p and syn.yaksynth_reads(p, half, READ_LEN, genome, 42, 0.005, 0.0005, j * half, 16) == nb
        bufs.append(p)

    def count(feeds, nb=nb):
        """(table, wall ms) of one unfiltered create pass over `feeds`, halves by index (their first nb bytes)"""
        t = yak_amd.Table(K, 10, 4, 0)
        L.yakamd_device_sync()
        t0 = time.perf_counter()
        assert L.yakamd_pass_begin(t.h, 1) == 0
        for i, j in enumerate(feeds):
            assert L.yakamd_feed_bases_host(t.h, bufs[j], nb, i * nb) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        return t, (time.perf_counter() - t0) * 1e3

    def timed(f):
        L.yakamd_device_sync()
        t0 = time.perf_counter()
        f()
        L.yakamd_device_sync()
        return (time.perf_counter() - t0) * 1e3

    small = 20000 * (READ_LEN + 1)                                    # warm-up: every call below once, on 20 k reads per side
    w0, w1, w2 = count([0], small)[0], count([1], small)[0], count([0, 1], small)[0]
    assert L.yakamd_ch_sum(w0.h, w1.h, 0) == 0, yak_amd._err()
    hw, w1.h = w1.h, None
    L.yak_ch_merge(w2.h, hw, 0, 1023, 4, 0)
    w0.close(); w2.close()
    out = {"reads": a.reads, "k": K}
    ta, out["count_first_half_ms"] = count([0])
    tb, out["count_second_half_ms"] = count([1])
    out["keys"] = [ta.tot, tb.tot]

    def do_sum():
        assert L.yakamd_ch_sum(ta.h, tb.h, 0) == 0, yak_amd._err()
    out["sum_ms"] = timed(do_sum)
    out["keys_sum"] = ta.tot
    if a.only != "sum":
        tw, out["recount_concatenation_ms"] = count([0, 1])
        J = yak_amd.inspect_tables(ta, tw)
        out["sum_equals_recount"] = bool(J.sum() == tw.tot == ta.tot and np.trace(J) == tw.tot)
        tw.close()
        ta.close()
        ta, _ = count([0])
        hb, tb.h = tb.h, None                                         # the merge frees its second table

        def do_merge():
            L.yak_ch_merge(ta.h, hb, 0, 1023, 4, 0)
        out["merge_0_1023_ms"] = timed(do_merge)
        out["keys_merge"] = ta.tot
    ta.close(); tb.close()
    for p in bufs:
        L.yakamd_host_free(p)
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
