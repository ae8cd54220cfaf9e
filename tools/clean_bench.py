"""Time `yak-amd clean` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37), beside tools/bubble_bench.py: yakamd_clean with both outputs to /dev/null end to end on a newly restored copy of
the table per call, with the eight parts of yakamd_clean_ms summed over its rounds; then, round by round on one more copy, yakamd_clean_round with
its parts and the forks, tips and simple bubbles of the graph before it; and, in the same run on the same table, the two yardsticks:
yakamd_bubbles -s to /dev/null, whose `find` step launches a comparable number of kernels over the same arrays as this layer's own (decisions and
image; compared on round 1, whose graph is the same), and yak_ch_shrink(1, 1023), the rebuild of the table that the drop table and the subtraction
do with a create pass in front.  --nofilter counts the reads in one pass without the bloom filter and keeps every k-mer.  A host clock around calls that end in a device synchronise; warm,
--reps calls, median and range.  The JSON goes to stdout and, as text, is appended to --out (profiles/clean_timing.txt).
Usage: python tools/clean_bench.py [--reads 10000000] [--reps 5] [--min-cnt 1] [--nofilter] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--nofilter", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.bubble as bubble
    import yak_amd.clean as clean
    import yak_amd.gfa as gfa
    import yak_amd.walk as walk
    L, BL, CL = yak_amd.lib(), bubble.lib(), clean.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads and syn.yaksynth_reads(h_reads, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb

    t = yak_amd.Table(K, 10, 4, 0 if a.nofilter else BF)
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

    def graph_of(tab):
        with walk.Walk(tab, a.min_cnt) as w, gfa.Gfa(w, K) as g, bubble.Bubbles(w, g, K) as b:
            ws, bs = w.stats(), b.stats()
            return dict(n_unitig=ws["n_open"] + ws["n_cycle"], n_fork=bs["n_fork"], n_tip=bs["n_tip"], n_bubble=bs["n_bubble"])

    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "table.yak").encode()
        assert L.yak_ch_dump(t.h, fn) == 0

        def copy():
            h = L.yak_ch_restore(fn)
            assert h, yak_amd._err()
            return yak_amd.Table(ptr=h)

        # the yardsticks on the table itself: bubbles -s, and the rebuild that removes nothing
        o = yak_amd.UgoptT()
        L.yakamd_ugopt_init(C.byref(o))
        o.min_cnt, o.stats_only = a.min_cnt, 1
        whole, find = [], []
        for i in range(a.reps + 1):                                    # the first call warms
            t0 = time.perf_counter()
            assert BL.yakamd_bubbles(C.byref(o), t.h, b"/dev/null") == 0, bubble._err()
            if i:
                whole.append((time.perf_counter() - t0) * 1e3); find.append(bubble.ms()[2])
        res["bubbles_s"] = dict(stat(whole), find=stat(find))
        shrink = []
        for i in range(a.reps + 1):
            c = copy()
            L.yakamd_device_sync()
            t0 = time.perf_counter()
            c.shrink(1, 1023)
            L.yakamd_device_sync()
            if i:
                shrink.append((time.perf_counter() - t0) * 1e3)
            c.close()
        res["shrink_1_1023"] = stat(shrink)
        t.close()

        # the command, end to end
        opt = clean.options(min_cnt=a.min_cnt)
        whole, parts, report = [], [], b""
        rep = os.path.join(d, "report.txt").encode()
        for i in range(a.reps + 1):
            c = copy()
            t0 = time.perf_counter()
            assert CL.yakamd_clean(C.byref(opt), c.h, b"/dev/null", rep if i == 0 else b"/dev/null") == 0, clean._err()
            if i:
                whole.append((time.perf_counter() - t0) * 1e3); parts.append(clean.ms())
            else:
                report = open(rep, "rb").read()
            c.close()
        res["clean"] = dict(stat(whole), parts={n: stat([p[j] for p in parts]) for j, n in enumerate(clean.MS_PARTS)})
        res["report"] = report.decode().splitlines()

        # round by round
        c = copy()
        res["rounds"] = []
        for r in range(opt.max_rounds):
            before = graph_of(c)
            rnd = clean.clean_round(c, a.min_cnt)
            res["rounds"].append(dict(before=before, round=rnd, ms=dict(zip(clean.MS_PARTS, [round(v, 3) for v in clean.ms()]))))
            if not rnd["removed"]:
                break
        c.close()
    # the comparisons are per round, on round 1: its graph is the one the yardsticks ran on
    own = [p[3] + p[4] for p in parts]
    res["own_kernels_all_rounds_ms"] = stat(own)
    first = res["rounds"][0]["ms"]
    res["own_round1_ms"] = round(first["decisions"] + first["image"], 3)
    res["own_round1_over_find"] = round(res["own_round1_ms"] / max(res["bubbles_s"]["find"]["median_ms"], 1e-9), 2)
    drop = [p[5] + p[6] for p in parts]
    res["drop_and_subtract_all_rounds_ms"] = stat(drop)
    res["drop_and_subtract_round1_ms"] = round(first["drop_table"] + first["subtract"], 3)
    res["drop_and_subtract_round1_over_shrink"] = round(res["drop_and_subtract_round1_ms"] / max(res["shrink_1_1023"]["median_ms"], 1e-9), 2)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads counted at k = %d, %s: %d stored keys; min_cnt = %d.\n"
                    % (a.reads, READ_LEN, K, "one pass without the filter, every k-mer kept" if a.nofilter else "-b%d, two passes" % BF, res["table_keys"], a.min_cnt))
            for ln in res["report"]:
                f.write("  " + ln + "\n")
            h = res["clean"]
            f.write("yakamd_clean (clean), both outputs to /dev/null   median %.1f ms (min %.1f, max %.1f), summed over its %d rounds:\n"
                    % (h["median_ms"], h["min_ms"], h["max_ms"], len(res["report"]) - 2))
            for s, v in h["parts"].items():
                f.write("  %-12s median %.2f ms (min %.2f, max %.2f)\n" % (s.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("round by round (yakamd_clean_round), the graph before the round and the parts of the round in ms:\n")
            for r, e in enumerate(res["rounds"], 1):
                b, m = e["before"], e["ms"]
                f.write("  round %d: %d unitigs, %d forks, %d tips, %d simple bubbles; removed %d k-mers (%d tips, %d arms); %s\n"
                        % (r, b["n_unitig"], b["n_fork"], b["n_tip"], b["n_bubble"], e["round"]["removed"], e["round"]["n_tip"], e["round"]["n_pop"],
                           ", ".join("%s %.2f" % (n.replace("_", " "), m[n]) for n in clean.MS_PARTS[:7])))
            v, w = res["own_kernels_all_rounds_ms"], res["bubbles_s"]
            f.write("this layer's own steps (decisions with the copies of the graph, image): all rounds median %.2f ms (min %.2f, max %.2f); round 1 %.2f ms\n"
                    % (v["median_ms"], v["min_ms"], v["max_ms"], res["own_round1_ms"]))
            f.write("yakamd_bubbles (bubbles) -s to /dev/null   median %.1f ms; its find step median %.2f ms (min %.2f, max %.2f): round 1's own steps / find = %.2f\n"
                    % (w["median_ms"], w["find"]["median_ms"], w["find"]["min_ms"], w["find"]["max_ms"], res["own_round1_over_find"]))
            v, w = res["drop_and_subtract_all_rounds_ms"], res["shrink_1_1023"]
            f.write("drop table + subtraction: all rounds median %.1f ms (min %.1f, max %.1f); round 1 %.2f ms; yak_ch_shrink(1, 1023) of the same table   median %.1f ms (min %.1f, max %.1f): "
                    "round 1 / shrink = %.2f\n\n" % (v["median_ms"], v["min_ms"], v["max_ms"], res["drop_and_subtract_round1_ms"], w["median_ms"], w["min_ms"], w["max_ms"],
                                                     res["drop_and_subtract_round1_over_shrink"]))


if __name__ == "__main__":
    main()
