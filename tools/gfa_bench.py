"""Time `yak-amd unitigs -G` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37), beside tools/walk_bench.py: yakamd_unitigs_gfa to /dev/null end to end, as GFA and with -s, with the walk's six
steps (yakamd_uwalk_ms) and the four of the links (yakamd_gfa_ms: the end table with the copies of the walk's results, the count and the scan, the
emit, the text with the copies out), the capacity of the end table and its longest probe walk, and, in the same run on the same table,
yakamd_unitigs_dev (`unitigs -g`) to /dev/null end to end.  --nofilter counts the reads in one pass without the bloom filter and keeps every
k-mer: the error k-mers make ends by the million.  A host clock around calls that end in a device synchronise; warm, --reps calls, median and
range.  The JSON goes to stdout and, as text, is appended to --out (profiles/gfa_timing.txt).
Usage: python tools/gfa_bench.py [--reads 10000000] [--reps 5] [--min-cnt 1] [--nofilter] [--out FILE]
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
WALK_STEPS = ("graph", "records_to_device", "ranking_rounds", "numbering_and_bases", "copies_out", "text")
GFA_STEPS = ("end_table", "count_and_scan", "emit", "text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--nofilter", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    L, WL, GL = yak_amd.lib(), walk.lib(), gfa.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb

    t = yak_amd.Table(K, 10, 4, 0 if a.nofilter else BF)
    # the benchmark's protocol: create pass, count pass, shrink; without the filter the one create pass counts every k-mer
    for create, again in (((1, False),) if a.nofilter else ((1, True), (0, False))):
        assert L.yakamd_pass_begin(t.h, create) == 0 and L.yakamd_feed_bases_host(t.h, h_reads, nb, 0) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        if again:
            t.destroy_bf(); t.clear()
    if not a.nofilter:
        t.shrink(2, 1023)
    L.yakamd_host_free(h_reads)
    res = {"reads": a.reads, "k": K, "bf_shift": 0 if a.nofilter else BF, "min_cnt": a.min_cnt, "table_keys": int(t.tot), "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    with walk.Walk(t, a.min_cnt) as w:                                 # warms, and gives the tallies
        res["walk_stats"] = w.stats()
        with gfa.Gfa(w, K) as g:
            res["gfa_stats"] = g.stats()
    o = yak_amd.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt = a.min_cnt

    def timed(call, reps):
        whole, wparts, gparts = [], [], []
        for i in range(reps + 1):                                      # the first call warms
            t0 = time.perf_counter()
            assert call() == 0, (yak_amd._err(), walk._err(), gfa._err())
            dt = (time.perf_counter() - t0) * 1e3
            wm, gm = (C.c_double * 6)(), (C.c_double * 4)()
            WL.yakamd_uwalk_ms(wm); GL.yakamd_gfa_ms(gm)
            if i:
                whole.append(dt); wparts.append(list(wm)); gparts.append(list(gm))
        return whole, wparts, gparts

    for stats_only, tag in ((1, "s"), (0, "text")):
        o.stats_only = stats_only
        whole, wparts, gparts = timed(lambda: GL.yakamd_unitigs_gfa(C.byref(o), t.h, b"/dev/null"), a.reps)
        res["unitigs_G_" + tag] = dict(stat(whole), walk={n: stat([p[j] for p in wparts]) for j, n in enumerate(WALK_STEPS[:4])},
                                       links={n: stat([p[j] for p in gparts]) for j, n in enumerate(GFA_STEPS)})
        whole, wparts, _ = timed(lambda: WL.yakamd_unitigs_dev(C.byref(o), t.h, b"/dev/null"), a.reps)
        res["unitigs_g_" + tag] = dict(stat(whole), walk={n: stat([p[j] for p in wparts]) for j, n in enumerate(WALK_STEPS)})
    t.close()
    print(json.dumps(res))
    if a.out:
        ws, gs = res["walk_stats"], res["gfa_stats"]
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads counted at k = %d, %s: %d stored keys; min_cnt = %d: %d nodes, %d open unitigs, %d cycles, %d bases.\n"
                    % (a.reads, READ_LEN, K, "one pass without the filter, every k-mer kept" if a.nofilter else "-b%d, two passes" % BF, res["table_keys"],
                       a.min_cnt, ws["n_node"], ws["n_open"], ws["n_cycle"], ws["sum_len"]))
            f.write("%d links; oriented ends of open unitigs with 0 .. 4 links: %s; end table %d slots, longest probe walk %d slots.\n"
                    % (gs["n_link"], " ".join("%d" % d for d in gs["end_deg"]), gs["table_slots"], gs["max_probe"]))
            for tag, label in (("s", "-s"), ("text", "text")):
                for name, steps in (("unitigs_G_", ("walk", "links")), ("unitigs_g_", ("walk",))):
                    h = res[name + tag]
                    f.write("%s %s to /dev/null   median %.1f ms (min %.1f, max %.1f)\n"
                            % ("yakamd_unitigs_gfa (unitigs -G)" if "G" in name else "yakamd_unitigs_dev (unitigs -g)", label, h["median_ms"], h["min_ms"], h["max_ms"]))
                    for part in steps:
                        for s, v in h[part].items():
                            f.write("  %-5s %-22s median %.1f ms (min %.1f, max %.1f)\n" % (part, s.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("\n")


if __name__ == "__main__":
    main()
