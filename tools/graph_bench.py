"""Time `yak-amd unitigs` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37): yakamd_graph_open with its three steps apart (the edge kernel's eight probes per node, the rank directory, the
link kernel's one probe per side of one edge; the test switch YAKAMD_GRAPH_TIMED puts a device synchronise between them), once with all eight
probes of a node requested together and once in two rounds of four (YAKAMD_GRAPH_INFLIGHT); a full pass of yakamd_graph_nodes_dev in ranges of 2^24
keys; and yakamd_unitigs -s to /dev/null end to end, with the graph, the records' way to the host, the host walk and the text apart.  A host clock
around calls that end in a device synchronise; warm, --reps calls, median and range.  The yardsticks beside the numbers: k_lookup's 44.9 G
lookups/s and mb_probe's 55 G random probes/s.  The JSON goes to stdout and, as text, to --out (profiles/graph_timing.txt).
Usage: python tools/graph_bench.py [--reads 10000000] [--reps 5] [--min-cnt 1] [--threads 8] [--out FILE]
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
READ_LEN, K, BF, PROBE_CEILING, LOOKUP_RATE = 150, 31, 37, 55e9, 44.9e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    L = yak_amd.lib()
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
    slots = sum(t.subtable(p)[0] for p in range(1 << 10))
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "min_cnt": a.min_cnt, "table_keys": keys, "table_slots": slots, "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    st = t.graph_stats(a.min_cnt)                                      # warms, and gives the number of probes
    res["stats"] = {key: st[key] for key in ("n_key", "n_node", "n_arc", "n_linked_side")}
    one_edge_sides = sum(st["deg"][l][r] * ((l == 1) + (r == 1)) for l in range(5) for r in range(5))
    res["one_edge_sides"] = one_edge_sides

    def opens(inflight, timed_steps):
        """--reps opens: the whole call's milliseconds, and its three steps' when they are timed apart"""
        L.yakamd_test_reset()
        L.yakamd_test_set(b"YAKAMD_GRAPH_INFLIGHT", inflight)
        if timed_steps:
            L.yakamd_test_set(b"YAKAMD_GRAPH_TIMED", 1)
        whole, steps = [], []
        for i in range(a.reps + 1):                                   # the first call warms
            t0 = time.perf_counter()
            g = L.yakamd_graph_open(t.h, a.min_cnt)
            dt = (time.perf_counter() - t0) * 1e3
            assert g, yak_amd._err()
            ms = (C.c_double * 3)()
            L.yakamd_graph_open_ms(g, ms)
            L.yakamd_graph_close(g)
            if i:
                whole.append(dt); steps.append(list(ms))
        L.yakamd_test_reset()
        return whole, steps

    for inflight in (8, 4):
        whole, _ = opens(inflight, False)
        _, steps = opens(inflight, True)
        e = statistics.median(s[0] for s in steps) / 1e3
        lk = statistics.median(s[2] for s in steps) / 1e3
        res["open_inflight_%d" % inflight] = dict(
            stat(whole), edges=stat([s[0] for s in steps]), rank=stat([s[1] for s in steps]), links=stat([s[2] for s in steps]),
            edge_probes_per_s=round(8 * st["n_node"] / e), edge_share_of_55G=round(8 * st["n_node"] / e / PROBE_CEILING, 4),
            link_probes_per_s=round(one_edge_sides / lk))

    g = L.yakamd_graph_open(t.h, a.min_cnt)
    assert g, yak_amd._err()
    P, batch = 1 << 10, 1 << 24
    sizes = [t.subtable(p)[1] for p in range(P)]
    ranges, lo, acc = [], 0, 0
    for p in range(P):
        if p > lo and acc + sizes[p] > batch:
            ranges.append((lo, p, acc)); lo, acc = p, 0
        acc += sizes[p]
    ranges.append((lo, P, acc))
    d = L.yakamd_dev_alloc(max(r[2] for r in ranges) * 32)
    assert d
    xs = []
    for i in range(a.reps + 1):
        t0 = time.perf_counter()
        for lo, hi, n in ranges:
            assert L.yakamd_graph_nodes_dev(g, lo, hi, d, n) == n, yak_amd._err()
        if i:
            xs.append((time.perf_counter() - t0) * 1e3)
    L.yakamd_dev_free(d)
    L.yakamd_graph_close(g)
    res["nodes_dev_full_pass"] = dict(stat(xs), ranges=len(ranges), records_per_s=round(keys / (statistics.median(xs) / 1e3)))

    o = yak_amd.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt, o.stats_only, o.n_threads = a.min_cnt, 1, a.threads
    whole, parts = [], []
    for i in range(3):
        t0 = time.perf_counter()
        assert L.yakamd_unitigs(C.byref(o), t.h, b"/dev/null") == 0, yak_amd._err()
        whole.append((time.perf_counter() - t0) * 1e3)
        ms = (C.c_double * 4)()
        L.yakamd_unitigs_ms(ms)
        parts.append(list(ms))
    res["unitigs_s_to_dev_null"] = dict(stat(whole), threads=a.threads, **{name: stat([p[j] for p in parts]) for j, name in enumerate(("graph", "records_to_host", "host_walk", "text"))})
    text = yak_amd._output_of("yakamd_unitigs", lambda out: L.yakamd_unitigs(C.byref(o), t.h, out)).decode()
    res["U_line"] = text.strip().split("\n")[-1].split("\t")[1:]
    t.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# yak-amd unitigs: timing on the benchmark's table (tools/graph_bench.py; DESIGN section 20)\n")
            f.write("One MI355X; %d x %d bp reads counted at k = %d, -b%d: %d stored keys in %d slots; min_cnt = %d: %d nodes, %d arcs, %d linked sides.\n"
                    % (a.reads, READ_LEN, K, BF, keys, slots, a.min_cnt, st["n_node"], st["n_arc"], st["n_linked_side"]))
            f.write("A host clock around calls that end in a device synchronise; the first call of each kind warms and is not counted; %d calls each.\n" % a.reps)
            f.write("Yardsticks (DESIGN section 7): k_lookup %.3g lookups/s, mb_probe %.3g random probes/s.\n\n" % (LOOKUP_RATE, PROBE_CEILING))
            for inflight in (8, 4):
                h = res["open_inflight_%d" % inflight]
                f.write("yakamd_graph_open, %s   median %.3f ms (min %.3f, max %.3f)\n"
                        % ("8 probes requested together " if inflight == 8 else "2 rounds of 4 probes         ", h["median_ms"], h["min_ms"], h["max_ms"]))
                for name, label in (("edges", "k_graph_edges"), ("rank", "k_graph_rank"), ("links", "k_graph_link, count")):
                    f.write("  %-20s median %.3f ms (min %.3f, max %.3f), with a synchronise behind it\n" % (label, h[name]["median_ms"], h[name]["min_ms"], h[name]["max_ms"]))
                f.write("  edge probes/s (8 per node)    %.3g = %.1f %% of mb_probe, %.1f %% of k_lookup\n"
                        % (h["edge_probes_per_s"], 100 * h["edge_share_of_55G"], 100 * h["edge_probes_per_s"] / LOOKUP_RATE))
                f.write("  link probes/s (%d sides of one edge)   %.3g\n" % (one_edge_sides, h["link_probes_per_s"]))
            h = res["nodes_dev_full_pass"]
            f.write("yakamd_graph_nodes_dev, all sub-tables in %d ranges   median %.3f ms (min %.3f, max %.3f): %.3g records/s\n"
                    % (h["ranges"], h["median_ms"], h["min_ms"], h["max_ms"], h["records_per_s"]))
            h = res["unitigs_s_to_dev_null"]
            f.write("yakamd_unitigs -s to /dev/null, %d threads, 3 calls   median %.1f ms (min %.1f, max %.1f)\n" % (a.threads, h["median_ms"], h["min_ms"], h["max_ms"]))
            for name, label in (("graph", "the graph"), ("records_to_host", "records to the host"), ("host_walk", "the host walk"), ("text", "the text")):
                f.write("  %-22s median %.1f ms (min %.1f, max %.1f)\n" % (label, h[name]["median_ms"], h[name]["min_ms"], h[name]["max_ms"]))
            f.write("  U line (open, cycles, bases, longest, N50)   %s\n" % " ".join(res["U_line"]))


if __name__ == "__main__":
    main()
