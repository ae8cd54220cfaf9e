"""Time the homopolymer compression on the benchmark's reads (bench.py: 10 M x 150 bp, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %) and
on a long-sequence image (the first --long-reads reads joined to one record), everything resident on the device:
  * yakamd_hpc_dev and yakamd_hpc_packed_dev, each beside a device-to-device copy of the same input bytes (the yardstick: a compaction reads its
    input once and writes at most one byte per position, a copy reads and writes the input's bytes); per call a host clock around a call that ends
    in a device synchronise, warm, --reps calls, median and range; the ASCII form also with the remap of the image's sequences;
  * the two-pass protocol (`yak count -k31 -b37`: create pass, count pass, shrink) through yakamd_count_hpc on the raw FASTA, beside yak_count of the
    same file (what the compaction adds to a count) and beside yak_count of the host-compressed file (what the user had to do before: the time of
    the host compression itself, one thread, is reported next to it).  The compressed FASTA is the compressed image with a header line per record,
    so a read with an N is two records there; its k-mers are the same.
The JSON goes to stdout and, as text, to --out (profiles/hpc_timing.txt).
Usage: python tools/hpc_bench.py [--reads 10000000] [--long-reads 1000000] [--reps 7] [--out FILE] [--no-e2e]
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
READ_LEN, K, BF = 150, 31, 37


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
    hip = C.CDLL("libamdhip64.so")                                     # the runtime the library itself runs on: the yardstick copy
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb
    reads = np.ctypeslib.as_array(C.cast(h_reads, C.POINTER(C.c_uint8)), (nb,))
    res = {"reads": a.reads, "reps": a.reps, "images": {}, "count": {}}

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
            assert call() >= 0, yak_amd._err()
            if i:
                xs.append(time.perf_counter() - t0)
        return xs

    def copy(dst, src, n):
        assert hip.hipMemcpy(dst, src, n, 3) == 0 and hip.hipDeviceSynchronize() == 0    # hipMemcpyDeviceToDevice
        return 0

    long_rec = np.ascontiguousarray(reads[: a.long_reads * (READ_LEN + 1)].reshape(-1, READ_LEN + 1)[:, :READ_LEN]).reshape(-1)
    layouts = {"reads": (reads, np.arange(a.reads, dtype=np.uint64) * (READ_LEN + 1), np.full(a.reads, READ_LEN, np.uint32)),
               "long": (np.concatenate((long_rec, np.full(1, 10, np.uint8))), np.zeros(1, np.uint64), np.array([len(long_rec)], np.uint32))}
    for name, (img, off, ln) in layouts.items():
        n = len(img)
        room = (n + 15) // 16 * 16
        nw = (n + 31) // 32
        d_img, d_off, d_len = put(np.concatenate((img, np.full(room - n, 10, np.uint8)))), put(off), put(ln)
        d_out, d_oo, d_lo = L.yakamd_dev_alloc(room), L.yakamd_dev_alloc(8 * len(off)), L.yakamd_dev_alloc(4 * len(off))
        d_codes, d_valid, d_copy = L.yakamd_dev_alloc(8 * nw + 16), L.yakamd_dev_alloc(4 * nw + 16), L.yakamd_dev_alloc(room)
        assert d_out and d_oo and d_lo and d_codes and d_valid and d_copy
        assert L.yakamd_pack_bases_dev(d_img, n, d_codes, d_valid, None) == 0 and L.yakamd_device_sync() == 0
        n_out = L.yakamd_hpc_dev(d_img, n, d_out, None, None, 0, None, None, None)
        assert n_out > 0 and L.yakamd_hpc_packed_dev(d_codes, d_valid, n, d_copy, None) == n_out, yak_amd._err()
        row = {"positions": n, "kept": int(n_out), "sequences": len(off)}
        row["ascii"] = stat(timed(lambda: L.yakamd_hpc_dev(d_img, n, d_out, None, None, 0, None, None, None)))
        row["ascii_with_remap"] = stat(timed(lambda: L.yakamd_hpc_dev(d_img, n, d_out, d_off, d_len, len(off), d_oo, d_lo, None)))
        row["copy_of_the_ascii_bytes"] = stat(timed(lambda: copy(d_copy, d_img, n)))
        row["packed"] = stat(timed(lambda: L.yakamd_hpc_packed_dev(d_codes, d_valid, n, d_out, None)))
        row["copy_of_the_packed_bytes"] = stat(timed(lambda: copy(d_copy, d_codes, 8 * nw) or copy(d_out, d_valid, 4 * nw)))
        for form, moved in (("ascii", n + n_out), ("packed", 12 * nw + n_out)):
            row[form]["GBps_read_plus_written"] = round(moved / (row[form]["median_ms"] * 1e-3) / 1e9, 1)
        res["images"][name] = row
        for p in (d_img, d_off, d_len, d_out, d_oo, d_lo, d_codes, d_valid, d_copy):
            L.yakamd_dev_free(p)

    if not a.no_e2e:
        with tempfile.TemporaryDirectory(prefix="hpc_bench_") as d:
            raw, comp = os.path.join(d, "raw.fa"), os.path.join(d, "comp.fa")
            img = reads.tobytes()
            t0 = time.perf_counter()
            cbuf = C.create_string_buffer((nb + 15) // 16 * 16)
            n_out = L.yakamd_hpc_host(img, nb, cbuf)
            res["count"]["host_compression_one_thread_s"] = round(time.perf_counter() - t0, 3)
            with open(raw, "wb") as f:
                f.write(b">r\n" + img.replace(b"\n", b"\n>r\n")[:-3])
            with open(comp, "wb") as f:
                f.write(b">r\n" + cbuf.raw[:n_out].replace(b"\n", b"\n>r\n")[:-3])
            del img, cbuf

            def protocol(count, fn):
                o = yak_amd.CoptT(); L.yak_copt_init(C.byref(o)); o.k, o.bf_shift = K, BF
                t0 = time.perf_counter()
                h = count(fn.encode(), C.byref(o), None)
                assert h, yak_amd._err()
                L.yak_ch_destroy_bf(h); L.yak_ch_clear(h, 1)
                assert count(fn.encode(), C.byref(o), h), yak_amd._err()
                L.yak_ch_shrink(h, 2, 1023, 1)
                dt = time.perf_counter() - t0
                tot = h.contents.tot
                L.yak_ch_destroy(h)
                return dt, int(tot)

            for tag, count, fn in (("yak_count_raw", L.yak_count, raw), ("yakamd_count_hpc_raw", L.yakamd_count_hpc, raw), ("yak_count_host_compressed", L.yak_count, comp)):
                runs = [protocol(count, fn) for _ in range(4)]          # the first run warms (runtime, pool, page cache)
                res["count"][tag] = {"s": [round(x, 3) for x, _ in runs[1:]], "keys": runs[-1][1]}
            assert res["count"]["yakamd_count_hpc_raw"]["keys"] == res["count"]["yak_count_host_compressed"]["keys"]
    L.yakamd_host_free(h_reads)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
