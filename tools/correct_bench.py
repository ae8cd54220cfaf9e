"""Time `yak-amd correct` on synthetic reads (tools/libyaksynth.so: reads of 150 bases at 30-fold coverage, seed 42, error rate 0.5 %, N rate
0.05 %, counted in one pass at k = 31 without the filter): yakamd_correct end to end with both outputs to /dev/null and the six parts of
yakamd_correct_ms, beside yakamd_lookup_dev alone on the same chunks of the same reads in the same process -- the yardstick: the command is
expected to cost about two lookups and its text.  The two are alternated, one call each per repetition, after one warm-up of both; a host clock
around calls that end in a device synchronise; median and range.  The JSON goes to stdout and, as text, is appended to --out
(profiles/correct_timing.txt).
Usage: python tools/correct_bench.py [--reads 2000000] [--reps 5] [--min-cnt 3] [--chunk 268435456] [--out FILE]
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
READ_LEN, K = 150, 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cnt", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.correct as correct
    L, CL = yak_amd.lib(), correct.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    syn = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    syn.yaksynth_reads.restype = C.c_int64
    syn.yaksynth_reads.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_int]
    nb = a.reads * (READ_LEN + 1)
    buf = C.create_string_buffer(nb)
    assert syn.yaksynth_reads(buf, a.reads, READ_LEN, 5 * a.reads, 42, 0.005, 0.0005, 0, 16) == nb
    t = yak_amd.Table(K, 10, 4, 0)
    t.count_pass_host(1, buf.raw)
    res = {"reads": a.reads, "k": K, "min_cnt": a.min_cnt, "chunk_size": a.chunk, "table_keys": int(t.tot), "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    # the chunks as the command cuts them: whole reads until their bases reach the chunk size; each on the device once, with room for its counts
    per = max(1, -(-a.chunk // READ_LEN))
    chunks = []
    for r0 in range(0, a.reads, per):
        n = (min(a.reads, r0 + per) - r0) * (READ_LEN + 1)
        room = (n + 15) & ~15
        d_img, d_cnt = L.yakamd_dev_alloc(room), L.yakamd_dev_alloc(2 * room)
        assert d_img and d_cnt, yak_amd._err()
        piece = buf.raw[r0 * (READ_LEN + 1):r0 * (READ_LEN + 1) + n] + b"\n" * (room - n)
        assert L.yakamd_memcpy_h2d(d_img, piece, room) == 0
        chunks.append((d_img, d_cnt, n))

    def lookups():
        t0 = time.perf_counter()
        for d_img, d_cnt, n in chunks:
            assert L.yakamd_lookup_dev(t.h, d_img, n, d_cnt) == 0, yak_amd._err()
        return (time.perf_counter() - t0) * 1e3

    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        with open(fa, "wb") as f:
            for i, r in enumerate(buf.raw.split(b"\n")[:-1]):
                f.write(b">r%d\n%s\n" % (i, r))
        rep = os.path.join(d, "report.txt")
        opt = correct.options(min_cnt=a.min_cnt, chunk_size=a.chunk)

        def command(report_fn):
            t0 = time.perf_counter()
            assert CL.yakamd_correct(C.byref(opt), t.h, fa.encode(), b"/dev/null", report_fn.encode()) == 0, correct._err()
            return (time.perf_counter() - t0) * 1e3, correct.ms()

        command(rep); lookups()                                      # warm
        res["report_last_line"] = open(rep, "rb").read().decode().splitlines()[-1]
        whole, parts, look = [], [], []
        for _ in range(a.reps):
            w, p = command("/dev/null")
            whole.append(w); parts.append(p); look.append(lookups())
    for d_img, d_cnt, n in chunks:
        L.yakamd_dev_free(d_img); L.yakamd_dev_free(d_cnt)
    t.close()
    res["correct"] = dict(stat(whole), parts={n: stat([p[j] for p in parts]) for j, n in enumerate(correct.MS_PARTS)})
    res["device_parts"] = stat([sum(p[:5]) for p in parts])
    res["lookup_alone"] = stat(look)
    res["correct_over_lookup"] = round(res["correct"]["median_ms"] / max(res["lookup_alone"]["median_ms"], 1e-9), 2)
    res["device_parts_over_lookup"] = round(res["device_parts"]["median_ms"] / max(res["lookup_alone"]["median_ms"], 1e-9), 2)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write("%d x %d bp reads, error rate 0.5 %%, counted at k = %d in one pass without the filter: %d stored keys; min_cnt = %d, %d chunk(s) of %d bases; %d repetitions after one warm-up.\n"
                    % (a.reads, READ_LEN, K, res["table_keys"], a.min_cnt, len(chunks), a.chunk, a.reps))
            f.write("  " + res["report_last_line"] + "\n")
            h = res["correct"]
            f.write("yakamd_correct (correct) from a FASTA file, both outputs to /dev/null   median %.1f ms (min %.1f, max %.1f):\n" % (h["median_ms"], h["min_ms"], h["max_ms"]))
            for s, v in h["parts"].items():
                f.write("  %-14s median %.2f ms (min %.2f, max %.2f)\n" % (s.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            v, w = res["device_parts"], res["lookup_alone"]
            f.write("its five device parts together   median %.2f ms (min %.2f, max %.2f)\n" % (v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("yakamd_lookup_dev alone on the same chunks, resident on the device   median %.2f ms (min %.2f, max %.2f): device parts / lookup = %.2f, command / lookup = %.2f\n\n"
                    % (w["median_ms"], w["min_ms"], w["max_ms"], res["device_parts_over_lookup"], res["correct_over_lookup"]))


if __name__ == "__main__":
    main()
