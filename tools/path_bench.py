"""Time `yak-amd paths` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37), beside tools/gfa_bench.py.  Two sets of sequences: the first --seq-reads of the benchmark's reads, and the
table's own unitigs, one sequence each.  Per set, on an image that lies in device memory: yakamd_path_hits_dev, the counting call and the writing
call of yakamd_path_chain_dev, and, in the same run on the same image, yakamd_lookup_dev -- the existing kernel that does the comparable probe per
position, the yardstick for k_path_hits.  Then yakamd_paths end to end on the unitigs as a FASTA file, to /dev/null, with the six parts of
yakamd_path_ms: the index, and summed over the chunks the hits, the count and the scan, the emit, the copies, the text.  A host clock around calls
that end in a device synchronise; warm, --reps calls, median and range.  The JSON goes to stdout and, as text, is appended to --out
(profiles/path_timing.txt).
Usage: python tools/path_bench.py [--reads 10000000] [--seq-reads 2000000] [--reps 5] [--min-cnt 1] [--out FILE]
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
PARTS = ("index", "hits", "count_and_scan", "emit", "copies", "text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--seq-reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    import yak_amd.path as path
    import yak_amd.walk as walk
    L, PL = yak_amd.lib(), path.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb
    t = yak_amd.Table(K, 10, 4, BF)
    for create, again in ((1, True), (0, False)):                      # the benchmark's protocol: create pass, count pass, shrink
        assert L.yakamd_pass_begin(t.h, create) == 0 and L.yakamd_feed_bases_host(t.h, h_reads, nb, 0) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        if again:
            t.destroy_bf(); t.clear()
    t.shrink(2, 1023)
    n_seq_reads = min(a.seq_reads, a.reads)
    reads_img = C.string_at(h_reads, n_seq_reads * (READ_LEN + 1))
    L.yakamd_host_free(h_reads)
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "min_cnt": a.min_cnt, "table_keys": int(t.tot), "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    def timed(call, ok=(0,)):
        out = []
        for i in range(a.reps + 1):                                    # the first call warms
            t0 = time.perf_counter()
            rc = call()
            L.yakamd_device_sync()
            dt = (time.perf_counter() - t0) * 1e3
            assert rc in ok, (rc, yak_amd._err(), path._err())
            if i:
                out.append(dt)
        return stat(out)

    with walk.Walk(t, a.min_cnt) as w:
        res["walk_stats"] = w.stats()
        desc, bases = w.desc(), w.bases()
        opens = []
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            px = path.Path(w, K)
            if i:
                opens.append((time.perf_counter() - t0) * 1e3)
            if i < a.reps:
                px.close()
        res["open"] = dict(stat(opens), index_ms=round(path.ms()[0], 3))
    # the unitigs, one sequence each
    n_u = len(desc)
    uoff = (desc["off"] + np.arange(n_u, dtype=np.uint64)).astype(np.uint64)
    ulen = (desc["n_node"] + np.uint64(K - 1)).astype(np.uint32)
    uimg = np.full(len(bases) + n_u, ord("\n"), np.uint8)
    keep = np.ones(len(uimg), bool)
    keep[(uoff + ulen.astype(np.uint64)).astype(np.int64)] = False
    uimg[keep] = bases
    roff = np.arange(n_seq_reads, dtype=np.uint64) * np.uint64(READ_LEN + 1)
    rlen = np.full(n_seq_reads, READ_LEN, np.uint32)
    try:
        for tag, img, off, ln in (("reads", reads_img, roff, rlen), ("unitigs", uimg.tobytes(), uoff, ulen)):
            n, n_seq = len(img), len(off)
            n16 = (n + 15) & ~15
            with path._Dev(L) as dev:
                d_img = dev.alloc(n16, img + b"\n" * (n16 - n))
                d_hit, d_u16 = dev.alloc(n16 * 8), dev.alloc(n16 * 2)
                d_off, d_len, d_tally = dev.alloc(n_seq * 8, off.tobytes()), dev.alloc(n_seq * 4, ln.tobytes()), dev.alloc(n_seq * 16)
                n_out = (C.c_int64 * 2)()
                r = {"bytes": n, "n_seq": n_seq}
                r["lookup_dev"] = timed(lambda: L.yakamd_lookup_dev(t.h, d_img, n, d_u16))
                r["hits"] = timed(lambda: PL.yakamd_path_hits_dev(px.px, d_img, n, d_hit))
                r["count_call"] = timed(lambda: PL.yakamd_path_chain_dev(px.px, d_hit, n, d_off, d_len, n_seq, None, 0, None, 0, d_tally, n_out), ok=(0, 1))
                r["n_path"], r["n_step"] = int(n_out[0]), int(n_out[1])
                d_paths, d_steps = dev.alloc(n_out[0] * 32), dev.alloc(n_out[1] * 8)
                r["write_call"] = timed(lambda: PL.yakamd_path_chain_dev(px.px, d_hit, n, d_off, d_len, n_seq, d_paths, n_out[0], d_steps, n_out[1], None, n_out))
                tal = dev.fetch(d_tally, np.zeros(n_seq, path.TALLY_DTYPE))
                r["n_kmer"], r["n_hit"] = int(tal["n_kmer"].sum(dtype=np.uint64)), int(tal["n_hit"].sum(dtype=np.uint64))
                for f in ("lookup_dev", "hits"):
                    r[f]["ns_per_position"] = round(r[f]["median_ms"] * 1e6 / n, 4)
            res[tag] = r
        res["path_stats"] = px.stats()
    finally:
        px.close()
    # end to end on the unitigs as a file
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "unitigs.fa")
        o = yak_amd.UgoptT()
        L.yakamd_ugopt_init(C.byref(o))
        o.min_cnt = a.min_cnt
        assert walk.lib().yakamd_unitigs_dev(C.byref(o), t.h, fa.encode()) == 0
        po = path.PpoptT()
        PL.yakamd_ppopt_init(C.byref(po))
        po.min_cnt = a.min_cnt
        whole, parts = [], []
        for i in range(3):
            t0 = time.perf_counter()
            assert PL.yakamd_paths(C.byref(po), t.h, fa.encode(), b"/dev/null") == 0, path._err()
            if i:
                whole.append((time.perf_counter() - t0) * 1e3)
                parts.append(path.ms())
        res["paths_on_unitigs"] = dict(stat(whole), parts={p: stat([x[j] for x in parts]) for j, p in enumerate(PARTS)})
    t.close()
    print(json.dumps(res))
    if a.out:
        ws, ps = res["walk_stats"], res["path_stats"]
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads counted at k = %d, -b%d, two passes: %d stored keys; min_cnt = %d: %d nodes, %d unitigs, %d bases.\n"
                    % (a.reads, READ_LEN, K, BF, res["table_keys"], a.min_cnt, ws["n_node"], ws["n_open"] + ws["n_cycle"], ws["sum_len"]))
            f.write("index %d slots (%d bytes), longest probe walk %d slots; yakamd_path_open median %.1f ms (min %.1f, max %.1f), of the last call %.1f ms on the index\n"
                    % (ps["table_slots"], 16 * ps["table_slots"], ps["max_probe"], res["open"]["median_ms"], res["open"]["min_ms"], res["open"]["max_ms"], res["open"]["index_ms"]))
            for tag in ("reads", "unitigs"):
                r = res[tag]
                f.write("%s: %d sequences, %d bytes, %d k-mers, %d hits, %d paths, %d steps\n" % (tag, r["n_seq"], r["bytes"], r["n_kmer"], r["n_hit"], r["n_path"], r["n_step"]))
                for name, key in (("yakamd_lookup_dev", "lookup_dev"), ("yakamd_path_hits_dev", "hits"), ("chain, counting call", "count_call"), ("chain, writing call", "write_call")):
                    v = r[key]
                    f.write("  %-22s median %.2f ms (min %.2f, max %.2f)%s\n" % (name, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                                 "  %.4f ns a position" % v["ns_per_position"] if "ns_per_position" in v else ""))
            h = res["paths_on_unitigs"]
            f.write("yakamd_paths on the unitigs as FASTA, to /dev/null   median %.1f ms (min %.1f, max %.1f)\n" % (h["median_ms"], h["min_ms"], h["max_ms"]))
            for p, v in h["parts"].items():
                f.write("  %-16s median %.1f ms (min %.1f, max %.1f)\n" % (p.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("\n")


if __name__ == "__main__":
    main()
