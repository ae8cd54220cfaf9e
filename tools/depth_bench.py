"""Time `yak-amd depth` against the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with
the two-pass protocol at k = 31, -b37) in two shapes: the reads themselves at w = 0 (10 M tiny windows), and the first reads joined to one
record (--long-reads of them, 150 Mb by default) at w = 0 and w = 10000.  Per shape: the lookup export, the reduce export (each a host clock around
a call that ends in a device synchronise; warm, --reps calls, median and range), the reduction's 2 bytes per position as a share of the 8 TB/s
HBM peak, and the whole yakamd_depth call on a file to /dev/null.  Then the sweep behind the threshold between the two reduction paths: the
long record cut into windows of 256 ... 16384 starts, every window forced through the wave-per-window path (YAKAMD_DEPTH_LONG = 2^20) and through
the histogram path (YAKAMD_DEPTH_LONG = 1).  The JSON goes to stdout and, as text, to --out (profiles/depth_timing.txt).
Usage: python tools/depth_bench.py [--reads 10000000] [--long-reads 1000000] [--reps 7] [--out FILE] [--no-e2e]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN, K, BF, HBM_PEAK = 150, 31, 37, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
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
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "table_keys": int(t.tot), "reps": a.reps, "shapes": {}, "sweep": []}

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

    def woff_of(lens, w):
        nw = np.ones(len(lens), np.uint64) if w == 0 else np.maximum(1, (lens.astype(np.uint64) + np.uint64(w - 1)) // np.uint64(w))
        return np.concatenate((np.zeros(1, np.uint64), np.cumsum(nw, dtype=np.uint64)))

    long_rec = np.ascontiguousarray(reads[: a.long_reads * (READ_LEN + 1)].reshape(-1, READ_LEN + 1)[:, :READ_LEN]).reshape(-1)
    layouts = {"reads": (reads, np.arange(a.reads, dtype=np.uint64) * (READ_LEN + 1), np.full(a.reads, READ_LEN, np.uint32)),
               "long": (np.concatenate((long_rec, np.full(1, 10, np.uint8))), np.zeros(1, np.uint64), np.array([len(long_rec)], np.uint32))}
    for name, ws in (("reads", [0]), ("long", [0, 10000])):
        img, off, ln = layouts[name]
        n_bytes = len(img)
        img16 = np.concatenate((img, np.full(-n_bytes % 16, 10, np.uint8)))
        d_img, d_off, d_len = put(img16), put(off), put(ln)
        d_t = L.yakamd_dev_alloc(len(img16) * 2)
        assert d_t
        lk = timed(lambda: L.yakamd_lookup_dev(t.h, d_img, n_bytes, d_t))
        for w in ws:
            woff = woff_of(ln, w)
            d_woff, d_win = put(woff), L.yakamd_dev_alloc(int(woff[-1]) * 24 + 16)
            assert d_win
            rd = timed(lambda: L.yakamd_depth_reduce_dev(K, w, d_t, d_off, d_len, d_woff, len(ln), n_bytes, d_win, None))
            med = statistics.median(rd)
            res["shapes"]["%s_w%d" % (name, w)] = {
                "sequences": len(ln), "positions": n_bytes, "windows": int(woff[-1]), "lookup": stat(lk), "reduce": stat(rd),
                "reduce_over_lookup": round(med / statistics.median(lk), 4),
                "reduce_GBps_at_2B_per_position": round(2 * n_bytes / med / 1e9, 1), "reduce_share_of_hbm_peak": round(2 * n_bytes / med / HBM_PEAK, 4)}
            if name == "long" and w == 0:                              # the sweep: same array, other windows, both paths forced
                for sw in (256, 512, 1024, 2048, 4096, 8192, 10000, 16384):
                    so = woff_of(ln, sw)
                    d_so, d_sw = put(so), L.yakamd_dev_alloc(int(so[-1]) * 24 + 16)
                    row = {"w": sw, "windows": int(so[-1])}
                    for tag, T in (("wave_per_window", 1 << 20), ("histogram", 1)):
                        L.yakamd_test_set(b"YAKAMD_DEPTH_LONG", T)
                        row[tag] = stat(timed(lambda: L.yakamd_depth_reduce_dev(K, sw, d_t, d_off, d_len, d_so, len(ln), n_bytes, d_sw, None)))
                    L.yakamd_test_reset()
                    res["sweep"].append(row)
                    L.yakamd_dev_free(d_so); L.yakamd_dev_free(d_sw)
            L.yakamd_dev_free(d_woff); L.yakamd_dev_free(d_win)
        for p in (d_img, d_off, d_len, d_t):
            L.yakamd_dev_free(p)

    if not a.no_e2e:                                                   # the whole call: file in, lines to /dev/null
        with tempfile.TemporaryDirectory(prefix="depth_bench_") as d:
            rows = reads.reshape(-1, READ_LEN + 1)
            fa = {"reads": os.path.join(d, "reads.fa"), "long": os.path.join(d, "long.fa")}
            with open(fa["reads"], "wb") as f:                       # a fixed-width name per read
                rec = np.empty((a.reads, 9 + READ_LEN + 1), np.uint8)
                rec[:, 0] = ord(">"); rec[:, 8] = ord("\n"); rec[:, 9:] = rows
                idx = np.arange(a.reads)
                for c in range(7):
                    rec[:, 7 - c] = ord("0") + (idx // 10 ** c) % 10
                f.write(rec.tobytes())
            with open(fa["long"], "wb") as f:
                f.write(b">joined\n" + long_rec.tobytes() + b"\n")
            for name, w in (("reads", 0), ("long", 0), ("long", 10000)):
                o = yak_amd.DpoptT()
                L.yakamd_dpopt_init(C.byref(o))
                o.window = w
                xs = []
                for i in range(3):
                    t0 = time.perf_counter()
                    assert L.yakamd_depth(C.byref(o), t.h, fa[name].encode(), b"/dev/null") == 0, yak_amd._err()
                    xs.append(time.perf_counter() - t0)
                res["shapes"]["%s_w%d" % (name, w)]["yakamd_depth_to_dev_null_s"] = [round(x, 3) for x in xs]
    t.close()
    L.yakamd_host_free(h_reads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
