"""Time `yak-amd unitigs -g` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37), beside tools/graph_bench.py: yakamd_unitigs_dev -s to /dev/null end to end with its six steps apart (the graph,
the records into device memory, the doubling rounds, the numbering and the bases, the copies out, the text), the number of rounds and the bytes
that came out of device memory, and, in the same run on the same table, yakamd_unitigs -s with --threads host threads, whose steps are the graph,
the records' way to the host, the host walk and the text.  The FASTA of both routes to /dev/null as well.  A host clock around calls that end in a
device synchronise; warm, --reps calls, median and range.  The JSON goes to stdout and, as text, to --out (profiles/walk_timing.txt).
Usage: python tools/walk_bench.py [--reads 10000000] [--reps 5] [--min-cnt 1] [--threads 8] [--out FILE]
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
READ_LEN, K, BF = 150, 31, 37
DEV_STEPS = ("graph", "records_to_device", "ranking_rounds", "numbering_and_bases", "copies_out", "text")
HOST_STEPS = ("graph", "records_to_host", "host_walk", "text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.walk as walk
    L, WL = yak_amd.lib(), walk.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb

    t = yak_amd.Table(K, 10, 4, BF)                                    # the benchmark's protocol: create pass, count pass, shrink
    for create in (1, 0):
        assert L.yakamd_pass_begin(t.h, create) == 0 and L.yakamd_feed_bases_host(t.h, h_reads, nb, 0) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        if create:
            t.destroy_bf(); t.clear()
    t.shrink(2, 1023)
    L.yakamd_host_free(h_reads)
    keys = int(t.tot)
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "min_cnt": a.min_cnt, "table_keys": keys, "reps": a.reps, "threads": a.threads}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    with walk.Walk(t, a.min_cnt) as w:                                 # warms, and gives the tallies
        st = w.stats()
    res["walk_stats"] = st
    n_u = st["n_open"] + st["n_cycle"]
    # descriptors, the cycles' records and indices, a counter per round, the totals of each scan (a second one with cycles) and the two reads of the tallies
    res["bytes_out_stats"] = 32 * n_u + 40 * st["host_nodes"] + 8 * st["rounds"] + 16 * (2 if st["host_nodes"] else 1) + 2 * 32
    res["bytes_out_fasta"] = res["bytes_out_stats"] + st["sum_len"]
    res["map_bytes_on_device"] = 16 * st["n_key"]

    o = yak_amd.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt, o.n_threads = a.min_cnt, a.threads

    def timed(call, ms_of, n_ms, reps):
        whole, parts = [], []
        for i in range(reps + 1):                                      # the first call warms
            t0 = time.perf_counter()
            assert call() == 0, (yak_amd._err(), walk._err())
            dt = (time.perf_counter() - t0) * 1e3
            ms = (C.c_double * n_ms)()
            ms_of(ms)
            if i:
                whole.append(dt); parts.append(list(ms))
        return whole, parts

    for stats_only, tag in ((1, "s"), (0, "fasta")):
        o.stats_only = stats_only
        whole, parts = timed(lambda: WL.yakamd_unitigs_dev(C.byref(o), t.h, b"/dev/null"), WL.yakamd_uwalk_ms, 6, a.reps)
        res["device_route_" + tag] = dict(stat(whole), **{name: stat([p[j] for p in parts]) for j, name in enumerate(DEV_STEPS)})
        whole, parts = timed(lambda: L.yakamd_unitigs(C.byref(o), t.h, b"/dev/null"), L.yakamd_unitigs_ms, 4, a.reps if stats_only else 2)
        res["host_route_" + tag] = dict(stat(whole), **{name: stat([p[j] for p in parts]) for j, name in enumerate(HOST_STEPS)})
    o.stats_only = 1
    dev = yak_amd._output_of("yakamd_unitigs_dev", lambda out: WL.yakamd_unitigs_dev(C.byref(o), t.h, out))
    host = yak_amd._output_of("yakamd_unitigs", lambda out: L.yakamd_unitigs(C.byref(o), t.h, out))
    assert dev == host, "the two routes disagree"
    res["U_line"] = dev.decode().strip().split("\n")[-1].split("\t")[1:]
    res["device_below_host"] = res["device_route_s"]["median_ms"] < res["host_route_s"]["median_ms"]
    t.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# yak-amd unitigs -g: the walk on the device against the host walk, on the benchmark's table (tools/walk_bench.py; DESIGN section 21)\n")
            f.write("One MI355X; %d x %d bp reads counted at k = %d, -b%d: %d stored keys; min_cnt = %d: %d nodes, %d open unitigs, %d cycles, %d bases.\n"
                    % (a.reads, READ_LEN, K, BF, keys, a.min_cnt, st["n_node"], st["n_open"], st["n_cycle"], st["sum_len"]))
            f.write("A host clock around calls that end in a device synchronise; the first call of each kind warms and is not counted; both routes in this one run.\n")
            f.write("%d doubling rounds; %d records of nodes on cycles reached the host; out of device memory came %d bytes for -s and %d for the FASTA;\n"
                    "the map (%d bytes) stays on the device.  The -s texts of the two routes are the same bytes.\n\n"
                    % (st["rounds"], st["host_nodes"], res["bytes_out_stats"], res["bytes_out_fasta"], res["map_bytes_on_device"]))
            for tag, label in (("s", "-s"), ("fasta", "FASTA")):
                for route, steps, name in (("device_route_", DEV_STEPS, "yakamd_unitigs_dev"), ("host_route_", HOST_STEPS, "yakamd_unitigs, %d threads" % a.threads)):
                    h = res[route + tag]
                    f.write("%s %s to /dev/null   median %.1f ms (min %.1f, max %.1f)\n" % (name, label, h["median_ms"], h["min_ms"], h["max_ms"]))
                    for s in steps:
                        f.write("  %-22s median %.1f ms (min %.1f, max %.1f)\n" % (s.replace("_", " "), h[s]["median_ms"], h[s]["min_ms"], h[s]["max_ms"]))
            f.write("U line (open, cycles, bases, longest, N50)   %s\n" % " ".join(res["U_line"]))
            f.write("device route below host route (-s, medians): %s, %.1f ms against %.1f ms\n"
                    % (res["device_below_host"], res["device_route_s"]["median_ms"], res["host_route_s"]["median_ms"]))


if __name__ == "__main__":
    main()
