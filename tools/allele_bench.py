"""Time `yak-amd bubbles -r` beside `yak-amd paths` on the inputs of tools/path_bench.py (bench.py's reads: 150 bp, G = 5 x reads, seed 42, e = 0.5 %,
N = 0.05 %, counted with the two-pass protocol at k = 31, -b37, so every stored k-mer was seen twice or more: a table of uncleaned reads, with
bubbles).  The first --seq-reads reads go to a FASTA file; in one process, on the same table and the same file, yakamd_paths and yakamd_alleles run
with stats_only to /dev/null, then yakamd_bubbles.  The yardstick is the path layer's own time on the hits and the chain in the very run of
yakamd_alleles (yakamd_path_ms after it: the calls of yakamd_alleles add to the thread's parts); beside it the parts of yakamd_allele_ms, the
numbers of steps, observations and bubbles, and the end-to-end times.  A host clock around calls that end in a device synchronise; the first call
warms, --reps calls, median and range.  The JSON goes to stdout and, as text, is appended to --out (profiles/allele_timing.txt).
Usage: python tools/allele_bench.py [--reads 10000000] [--seq-reads 500000] [--reps 3] [--min-cnt 1] [--out FILE]
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
PATH_PARTS = ("index", "hits", "count_and_scan", "emit", "copies", "text")
ALLELE_PARTS = ("arm_map", "count_and_scan", "emit", "copies", "text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--seq-reads", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-cnt", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.allele as allele
    import yak_amd.bubble as bubble
    import yak_amd.path as path
    L, PL, AL, BL = yak_amd.lib(), path.lib(), allele.lib(), bubble.lib()
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
    n_seq = min(a.seq_reads, a.reads)
    lines = C.string_at(h_reads, n_seq * (READ_LEN + 1)).split(b"\n")[:n_seq]
    L.yakamd_host_free(h_reads)
    res = {"reads": a.reads, "seq_reads": n_seq, "k": K, "bf_shift": BF, "min_cnt": a.min_cnt, "table_keys": int(t.tot), "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    with tempfile.TemporaryDirectory() as d:
        fa, out = os.path.join(d, "reads.fa"), os.path.join(d, "out.txt")
        with open(fa, "wb") as f:
            f.write(b"".join(b">%d\n%s\n" % (i, s) for i, s in enumerate(lines)))
        del lines
        po = path.PpoptT()
        PL.yakamd_ppopt_init(C.byref(po))
        po.min_cnt, po.stats_only = a.min_cnt, 1
        ao = allele.AloptT()
        AL.yakamd_alopt_init(C.byref(ao))
        ao.min_cnt, ao.stats_only = a.min_cnt, 1
        uo = yak_amd.UgoptT()
        L.yakamd_ugopt_init(C.byref(uo))
        uo.min_cnt, uo.stats_only = a.min_cnt, 1
        runs = {"paths": [], "alleles": [], "bubbles": []}
        parts = {"paths": [], "alleles_path": [], "alleles": []}
        for i in range(a.reps + 1):                                    # the first round warms
            t0 = time.perf_counter()
            assert PL.yakamd_paths(C.byref(po), t.h, fa.encode(), b"/dev/null") == 0, path._err()
            t1 = time.perf_counter()
            p_ms = path.ms()
            assert AL.yakamd_alleles(C.byref(ao), t.h, fa.encode(), out.encode()) == 0, allele._err()
            t2 = time.perf_counter()
            ap_ms, a_ms = path.ms(), allele.ms()
            assert BL.yakamd_bubbles(C.byref(uo), t.h, b"/dev/null") == 0, bubble._err()
            t3 = time.perf_counter()
            if i:
                runs["paths"].append((t1 - t0) * 1e3); runs["alleles"].append((t2 - t1) * 1e3); runs["bubbles"].append((t3 - t2) * 1e3)
                parts["paths"].append(p_ms); parts["alleles_path"].append(ap_ms); parts["alleles"].append(a_ms)
        res["tail"] = open(out).read().splitlines()[-1].split("\t")
    t.close()
    res["end_to_end"] = {k: stat(v) for k, v in runs.items()}
    res["path_ms_in_paths"] = {p: stat([x[j] for x in parts["paths"]]) for j, p in enumerate(PATH_PARTS)}
    res["path_ms_in_alleles"] = {p: stat([x[j] for x in parts["alleles_path"]]) for j, p in enumerate(PATH_PARTS)}
    res["allele_ms"] = {p: stat([x[j] for x in parts["alleles"]]) for j, p in enumerate(ALLELE_PARTS)}
    pm, am = res["path_ms_in_alleles"], res["allele_ms"]
    yard = pm["hits"]["median_ms"] + pm["count_and_scan"]["median_ms"] + pm["emit"]["median_ms"]
    own = am["count_and_scan"]["median_ms"] + am["emit"]["median_ms"]
    res["yardstick_ms"], res["own_ms"], res["own_over_yardstick"] = round(yard, 3), round(own, 3), round(own / yard, 4) if yard else None
    print(json.dumps(res))
    if a.out:
        tl = res["tail"]
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads counted at k = %d, -b%d, two passes: %d stored keys; min_cnt = %d; the first %d reads as FASTA, stats_only, one process, %d rounds behind a warming one.\n"
                    % (a.reads, READ_LEN, K, BF, res["table_keys"], a.min_cnt, n_seq, a.reps))
            f.write("T line of yakamd_alleles: %s sequences, %s bases, %s paths, %s steps, %s observations (%s full), %s bubbles (het %s, hom1 %s, hom2 %s, none %s)\n"
                    % (tl[1], tl[2], tl[3], tl[4], tl[5], tl[6], tl[8], tl[9], tl[10], tl[11], tl[12]))
            for title, key, names in (("yakamd_path_ms after yakamd_paths", "path_ms_in_paths", PATH_PARTS), ("yakamd_path_ms after yakamd_alleles", "path_ms_in_alleles", PATH_PARTS),
                                      ("yakamd_allele_ms after yakamd_alleles", "allele_ms", ALLELE_PARTS)):
                f.write(title + "\n")
                for p in names:
                    v = res[key][p]
                    f.write("  %-16s median %.2f ms (min %.2f, max %.2f)\n" % (p.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("the path layer's hits and chain in yakamd_alleles %.2f ms; the allele kernels (count and scan twice, emit) %.2f ms: %.1f %% of it\n"
                    % (yard, own, 100.0 * own / yard if yard else 0.0))
            e = res["end_to_end"]
            f.write("end to end: yakamd_alleles median %.1f ms (min %.1f, max %.1f); yakamd_paths -s %.1f ms (min %.1f, max %.1f) and yakamd_bubbles -s %.1f ms (min %.1f, max %.1f) run separately: %.1f ms\n\n"
                    % (e["alleles"]["median_ms"], e["alleles"]["min_ms"], e["alleles"]["max_ms"], e["paths"]["median_ms"], e["paths"]["min_ms"], e["paths"]["max_ms"],
                       e["bubbles"]["median_ms"], e["bubbles"]["min_ms"], e["bubbles"]["max_ms"], e["paths"]["median_ms"] + e["bubbles"]["median_ms"]))


if __name__ == "__main__":
    main()
