"""Time `yak-amd bubbles` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37), beside tools/gfa_bench.py: yakamd_bubbles to /dev/null end to end, as B lines and with -s, with the five parts
of yakamd_bubble_ms (the copies of the walk's results and the links, the first link of every end, the find with its scan, the classification, the
text with the copies out), the links' below (yakamd_gfa_ms) and the walk's first four (yakamd_uwalk_ms), and, in the same run on the same
table, yakamd_unitigs_gfa (`unitigs -G`) with -s to /dev/null end to end: the yardstick.  --nofilter counts the reads in one pass without the
bloom filter and keeps every k-mer: the error k-mers make forks and tips by the million.  A host clock around calls that end in a device
synchronise; warm, --reps calls, median and range.  The JSON goes to stdout and, as text, is appended to --out (profiles/bubble_timing.txt).
Usage: python tools/bubble_bench.py [--reads 10000000] [--reps 5] [--min-cnt 1] [--nofilter] [--out FILE]
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
WALK_STEPS = ("graph", "records_to_device", "ranking_rounds", "numbering_and_bases")
GFA_STEPS = ("end_table", "count_and_scan", "emit", "text")
BUBBLE_STEPS = ("copies", "first_links", "find", "classify", "text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--nofilter", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.bubble as bubble
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    L, WL, GL, BL = yak_amd.lib(), walk.lib(), gfa.lib(), bubble.lib()
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
            with bubble.Bubbles(w, g, K) as b:
                res["bubble_stats"] = b.stats()
    o = yak_amd.UgoptT()
    L.yakamd_ugopt_init(C.byref(o))
    o.min_cnt = a.min_cnt

    def timed(call, reps):
        whole, wparts, gparts, bparts = [], [], [], []
        for i in range(reps + 1):                                      # the first call warms
            t0 = time.perf_counter()
            assert call() == 0, (yak_amd._err(), walk._err(), gfa._err(), bubble._err())
            dt = (time.perf_counter() - t0) * 1e3
            wm, gm = (C.c_double * 6)(), (C.c_double * 4)()
            WL.yakamd_uwalk_ms(wm); GL.yakamd_gfa_ms(gm)
            if i:
                whole.append(dt); wparts.append(list(wm)); gparts.append(list(gm)); bparts.append(bubble.ms())
        return whole, wparts, gparts, bparts

    for stats_only, tag in ((1, "s"), (0, "text")):
        o.stats_only = stats_only
        whole, wparts, gparts, bparts = timed(lambda: BL.yakamd_bubbles(C.byref(o), t.h, b"/dev/null"), a.reps)
        res["bubbles_" + tag] = dict(stat(whole), walk={n: stat([p[j] for p in wparts]) for j, n in enumerate(WALK_STEPS)},
                                     links={n: stat([p[j] for p in gparts]) for j, n in enumerate(GFA_STEPS[:3])},
                                     bubbles={n: stat([p[j] for p in bparts]) for j, n in enumerate(BUBBLE_STEPS)})
        if stats_only:
            whole, wparts, gparts, _ = timed(lambda: GL.yakamd_unitigs_gfa(C.byref(o), t.h, b"/dev/null"), a.reps)
            res["unitigs_G_s"] = dict(stat(whole), walk={n: stat([p[j] for p in wparts]) for j, n in enumerate(WALK_STEPS)},
                                      links={n: stat([p[j] for p in gparts]) for j, n in enumerate(GFA_STEPS)})
    t.close()
    print(json.dumps(res))
    if a.out:
        ws, gs, bs = res["walk_stats"], res["gfa_stats"], res["bubble_stats"]
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads counted at k = %d, %s: %d stored keys; min_cnt = %d: %d nodes, %d open unitigs, %d cycles, %d bases, %d links.\n"
                    % (a.reads, READ_LEN, K, "one pass without the filter, every k-mer kept" if a.nofilter else "-b%d, two passes" % BF, res["table_keys"],
                       a.min_cnt, ws["n_node"], ws["n_open"], ws["n_cycle"], ws["sum_len"], gs["n_link"]))
            f.write("%d bubbles (S %d, E %d, I %d) of %d forks; %d tips of %d nodes; the longest arm %d nodes.\n"
                    % (bs["n_bubble"], bs["n_type"][0], bs["n_type"][1], bs["n_type"][2], bs["n_fork"], bs["n_tip"], bs["tip_nodes"], bs["max_arm_nodes"]))
            for key, label in (("bubbles_s", "yakamd_bubbles (bubbles) -s"), ("unitigs_G_s", "yakamd_unitigs_gfa (unitigs -G) -s"), ("bubbles_text", "yakamd_bubbles (bubbles) text")):
                h = res[key]
                f.write("%s to /dev/null   median %.1f ms (min %.1f, max %.1f)\n" % (label, h["median_ms"], h["min_ms"], h["max_ms"]))
                for part in ("walk", "links", "bubbles"):
                    for s, v in h.get(part, {}).items():
                        f.write("  %-7s %-16s median %.2f ms (min %.2f, max %.2f)\n" % (part, s.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("\n")


if __name__ == "__main__":
    main()
