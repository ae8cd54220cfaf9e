"""Time `yak-amd cover` against the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with
the two-pass protocol at k = 31, -b37) on two resident chunks: the first reads joined to one record (--contig bases, 100 Mb by default) and
--short reads of 150 bp (1 M).  Per chunk: the lookup export, the cover export without a mask, with the soft and with the hard mask and without sequences (no tally), and the
`depth -w0` reduction (yakamd_depth_reduce_dev, which this change leaves as it was) -- each a host clock around a call that ends in a device
synchronise; warm, --reps calls, median and range -- then cover / lookup, and the bytes per position the pass moves (2 read and 1 written, with
a mask 3 and 2) as GB/s and as a share of the 8 TB/s HBM peak.  The JSON goes to stdout and, as text, to --out (profiles/cover_timing.txt).
Usage: python tools/cover_bench.py [--reads 10000000] [--contig 100000000] [--short 1000000] [--reps 7] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN, K, BF, HBM_PEAK = 150, 31, 37, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--contig", type=int, default=100_000_000)
    ap.add_argument("--short", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb
    reads = np.ctypeslib.as_array(C.cast(h_reads, C.POINTER(C.c_uint8)), (nb,))

    t = yak_amd.Table(K, 10, 4, BF)                                    # the benchmark's protocol: create pass, count pass, shrink
    for create in (1, 0):
        assert L.yakamd_pass_begin(t.h, create) == 0 and L.yakamd_feed_bases_host(t.h, h_reads, nb, 0) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        if create:
            t.destroy_bf(); t.clear()
    t.shrink(2, 1023)
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "table_keys": int(t.tot), "reps": a.reps, "predicate": "1:1023", "chunks": {}}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs) * 1e3, 3), "min_ms": round(min(xs) * 1e3, 3), "max_ms": round(max(xs) * 1e3, 3)}

    def put(arr):
        p = L.yakamd_dev_alloc(max(arr.nbytes, 16))
        assert p and L.yakamd_memcpy_h2d(p, arr.ctypes.data, arr.nbytes) == 0, yak_amd._err()
        return p

    def timed(call):
        xs = []
        for i in range(a.reps + 1):                                  # the first call warms
            t0 = time.perf_counter()
            assert call() == 0, yak_amd._err()
            if i:
                xs.append(time.perf_counter() - t0)
        return xs

    n_join = min(a.reads, (a.contig + READ_LEN - 1) // READ_LEN)
    contig = np.ascontiguousarray(reads[: n_join * (READ_LEN + 1)].reshape(-1, READ_LEN + 1)[:, :READ_LEN]).reshape(-1)[:a.contig]
    n_short = min(a.reads, a.short)
    layouts = {"contig": (np.concatenate((contig, np.full(1, 10, np.uint8))), np.zeros(1, np.uint64), np.array([len(contig)], np.uint32)),
               "reads": (reads[: n_short * (READ_LEN + 1)], np.arange(n_short, dtype=np.uint64) * (READ_LEN + 1), np.full(n_short, READ_LEN, np.uint32))}
    for name, (img, off, ln) in layouts.items():
        n_bytes = len(img)
        img16 = np.concatenate((img, np.full(-n_bytes % 16, 10, np.uint8)))
        d_img, d_off, d_len = put(img16), put(off), put(ln)
        d_t, d_cov, d_msk = L.yakamd_dev_alloc(len(img16) * 2), L.yakamd_dev_alloc(len(img16)), L.yakamd_dev_alloc(len(img16))
        d_tal, d_win = L.yakamd_dev_alloc(len(ln) * 16), L.yakamd_dev_alloc(len(ln) * 24 + 16)
        d_woff = put(np.arange(len(ln) + 1, dtype=np.uint64))        # w = 0: one window per sequence
        assert d_t and d_cov and d_msk and d_tal and d_win
        lk = timed(lambda: L.yakamd_lookup_dev(t.h, d_img, n_bytes, d_t))
        row = {"sequences": len(ln), "positions": n_bytes, "lookup": stat(lk)}
        for tag, mask, per_pos in (("cover", 0, 3), ("cover_soft", 1, 5), ("cover_hard", 2, 5)):
            xs = timed(lambda: L.yakamd_cover_dev(K, 1, 1023, d_t, n_bytes, d_off, d_len, len(ln), d_img, mask, d_cov, d_msk if mask else None, d_tal, None))
            med = statistics.median(xs)
            row[tag] = dict(stat(xs), over_lookup=round(med / statistics.median(lk), 4), bytes_per_position=per_pos,
                            GBps=round(per_pos * n_bytes / med / 1e9, 1), share_of_hbm_peak=round(per_pos * n_bytes / med / HBM_PEAK, 4))
        xs = timed(lambda: L.yakamd_cover_dev(K, 1, 1023, d_t, n_bytes, None, None, 0, None, 0, d_cov, None, None, None))
        row["cover_without_tally"] = dict(stat(xs), over_lookup=round(statistics.median(xs) / statistics.median(lk), 4))
        tal = np.empty(len(ln) * 4, np.uint32)
        assert L.yakamd_memcpy_d2h(tal.ctypes.data, d_tal, tal.nbytes) == 0
        row["covered_fraction"] = round(float(tal[2::4].sum(dtype=np.uint64)) / max(1, int(ln.sum(dtype=np.uint64))), 4)
        rd = timed(lambda: L.yakamd_depth_reduce_dev(K, 0, d_t, d_off, d_len, d_woff, len(ln), n_bytes, d_win, None))
        row["depth_w0_reduce"] = dict(stat(rd), over_lookup=round(statistics.median(rd) / statistics.median(lk), 4))
        res["chunks"][name] = row
        for p in (d_img, d_off, d_len, d_t, d_cov, d_msk, d_tal, d_win, d_woff):
            L.yakamd_dev_free(p)
    t.close()
    L.yakamd_host_free(h_reads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
