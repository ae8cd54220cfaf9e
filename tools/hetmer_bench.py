"""Time `yak-amd hetmers` on the benchmark's table (bench.py: 10 M x 150 bp reads, G = 50 M, seed 42, e = 0.5 %, N = 0.05 %, counted with the
two-pass protocol at k = 31, -b37): yakamd_hetmers_dev (a host clock around a call that ends in a device synchronise; warm, --reps calls, median
and range), the pair list export (the size query, then the call that writes the records) and the whole yakamd_hetmers call to /dev/null, without
and with the K lines.  Every stored key is a member at min_cnt = 1 and probes the table three times, so keys/s and probes/s = 3 keys/s follow; the
yardstick is the 55 G random probes/s of DESIGN section 7 (tests/tools/mb/mb_probe.hip).  The export's time includes staging the keys (the device
side .yak body of each range of sub-tables).  The JSON goes to stdout and, as text, to --out (profiles/hetmer_timing.txt).
Usage: python tools/hetmer_bench.py [--reads 10000000] [--reps 7] [--min-cnt 1] [--out FILE]
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
READ_LEN, K, BF, PROBE_CEILING = 150, 31, 37, 55e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-cnt", type=int, default=1)
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
    res = {"reads": a.reads, "k": K, "bf_shift": BF, "min_cnt": a.min_cnt, "table_keys": keys, "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs) * 1e3, 3), "min_ms": round(min(xs) * 1e3, 3), "max_ms": round(max(xs) * 1e3, 3)}

    def timed(call, reps):
        xs = []
        for i in range(reps + 1):                                    # the first call warms
            t0 = time.perf_counter()
            call()
            if i:
                xs.append(time.perf_counter() - t0)
        return xs

    n_tally = 1024 * 1024 * 8 + 64
    d_tally = L.yakamd_dev_alloc(n_tally)
    assert d_tally and L.yakamd_memcpy_h2d(d_tally, bytes(n_tally), n_tally) == 0

    def join():
        assert L.yakamd_hetmers_dev(t.h, a.min_cnt, d_tally, d_tally + 1024 * 1024 * 8, None) == 0, yak_amd._err()
    xs = timed(join, a.reps)
    L.yakamd_dev_free(d_tally)
    J, g = t.hetmers(a.min_cnt)
    members = sum(s * g[s] for s in range(5))
    med = statistics.median(xs)
    res["hetmers_dev"] = dict(stat(xs), members=members, groups=g[1:], pairs=sum(J.values()), keys_per_s=round(keys / med),
                              probes_per_s=round(3 * members / med), share_of_55G_probes=round(3 * members / med / PROBE_CEILING, 4))

    n_pairs = L.yakamd_hetmer_pairs_dev(t.h, a.min_cnt, None, 0)
    assert n_pairs == sum(J.values()), yak_amd._err()
    d_pairs = L.yakamd_dev_alloc(max(n_pairs, 1) * 24)
    assert d_pairs
    q = timed(lambda: L.yakamd_hetmer_pairs_dev(t.h, a.min_cnt, None, 0), 3)
    w = timed(lambda: L.yakamd_hetmer_pairs_dev(t.h, a.min_cnt, d_pairs, n_pairs), 3)
    L.yakamd_dev_free(d_pairs)
    res["pairs_dev"] = {"pairs": int(n_pairs), "size_query": stat(q), "write": stat(w)}

    o = yak_amd.HmoptT()
    L.yakamd_hmopt_init(C.byref(o))
    o.min_cnt = a.min_cnt
    for name, p in (("hetmers_to_dev_null", 0), ("hetmers_with_pairs_to_dev_null", 1)):
        o.print_pairs = p

        def whole():
            assert L.yakamd_hetmers(C.byref(o), t.h, b"/dev/null") == 0, yak_amd._err()
        res[name] = stat(timed(whole, 3))
    t.close()
    print(json.dumps(res))
    if a.out:
        h = res["hetmers_dev"]
        with open(a.out, "w") as f:
            f.write("# yak-amd hetmers: timing on the benchmark's table (tools/hetmer_bench.py; DESIGN section 17)\n")
            f.write("One MI355X; %d x %d bp reads counted at k = %d, -b%d: %d stored keys, all of them members at min_cnt = %d.\n"
                    % (a.reads, READ_LEN, K, BF, keys, a.min_cnt))
            f.write("A host clock around calls that end in a device synchronise; the first call of each kind warms and is not counted.\n\n")
            f.write("yakamd_hetmers_dev, %d calls         median %.3f ms (min %.3f, max %.3f), staging of the keys included\n"
                    % (a.reps, h["median_ms"], h["min_ms"], h["max_ms"]))
            f.write("  groups of 1 / 2 / 3 / 4 members    %d / %d / %d / %d; %d pairs\n" % (*h["groups"], h["pairs"]))
            f.write("  keys/s                             %.3g\n" % h["keys_per_s"])
            f.write("  probes/s (3 per member key)        %.3g = %.1f %% of the 55 G random probes/s of DESIGN section 7\n"
                    % (h["probes_per_s"], 100 * h["share_of_55G_probes"]))
            for name, label in (("size_query", "yakamd_hetmer_pairs_dev, size query "), ("write", "yakamd_hetmer_pairs_dev, %d records" % n_pairs)):
                s = res["pairs_dev"][name]
                f.write("%s   median %.3f ms (min %.3f, max %.3f), 3 calls\n" % (label, s["median_ms"], s["min_ms"], s["max_ms"]))
            for name, label in (("hetmers_to_dev_null", "yakamd_hetmers to /dev/null        "), ("hetmers_with_pairs_to_dev_null", "yakamd_hetmers -p to /dev/null     ")):
                s = res[name]
                f.write("%s   median %.3f ms (min %.3f, max %.3f), 3 calls\n" % (label, s["median_ms"], s["min_ms"], s["max_ms"]))


if __name__ == "__main__":
    main()
