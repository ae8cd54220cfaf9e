"""Time `yak-amd bubbles -r -p` beside `yak-amd bubbles -r` on a diploid input of its own making: a random genome of --genome bases and a copy with
a SNP every 60 to 90 bases, error-free reads of 150 bp from both at --cov-fold coverage each, every other read from the other strand, counted with
the two-pass protocol at k = 31, -b37.  The reads go to a FASTA file; in one process, on the same table and the same file, yakamd_alleles and
yakamd_phase run with stats_only, --reps rounds behind a warming one.  The yardstick is the path layer's own time on the hits and the chain in the
very run of yakamd_phase (yakamd_path_ms after it); beside it the parts of yakamd_phase_ms and of yakamd_allele_ms, the rounds of the solve, the
growths of the pair table and the sizes; end to end the yardstick is yakamd_alleles.  A host clock around calls that end in a device synchronise;
median and range.  The JSON goes to stdout and, as text, is appended to --out (profiles/phase_timing.txt); --keep DIR leaves reads.fa and
table.yak there.
Usage: python tools/phase_bench.py [--genome 5000000] [--cov 20] [--reps 3] [--seed 32] [--out FILE] [--keep DIR]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN, K, BF = 150, 31, 37
PATH_PARTS = ("index", "hits", "count_and_scan", "emit", "copies", "text")
ALLELE_PARTS = ("arm_map", "count_and_scan", "emit", "copies", "text")
PHASE_PARTS = ("compaction", "votes_and_growth", "solve", "copies", "text")


def diploid_reads(genome, cov, seed):
    """the reads as one image, each followed by a newline, and the number of SNPs"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, genome, dtype=np.uint8)
    pos = np.cumsum(rng.integers(60, 91, genome // 60))
    pos = pos[pos < genome - 60]
    b = a.copy()
    b[pos] = (a[pos] + rng.integers(1, 4, len(pos), dtype=np.uint8)) & 3
    n = genome * cov // READ_LEN                                  # per haplotype
    img = np.full((2 * n, READ_LEN + 1), ord("\n"), np.uint8)
    at = np.arange(READ_LEN)
    for h, hap in enumerate((a, b)):
        starts = rng.integers(0, genome - READ_LEN, n)
        rows = hap[starts[:, None] + at]
        rows[1::2] = 3 - rows[1::2, ::-1]                         # every other read from the other strand
        img[h::2, :READ_LEN] = np.frombuffer(b"ACGT", np.uint8)[rows]
    return img, len(pos)


def verbose_line(call):
    """what a call writes to stderr with YAKAMD_VERBOSE set: the library prints there, so the descriptor itself goes to a file for the call"""
    os.environ["YAKAMD_VERBOSE"] = "1"
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            del os.environ["YAKAMD_VERBOSE"]
        f.seek(0)
        return f.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--cov", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    import yak_amd
    import yak_amd.allele as allele
    import yak_amd.path as path
    import yak_amd.phase as phase
    L, AL, PHL = yak_amd.lib(), allele.lib(), phase.lib()
    path.lib()
    assert L.yakamd_device_count() >= 1, "no MI355X: nothing is measured"
    img, n_snp = diploid_reads(a.genome, a.cov, a.seed)
    n_reads, nb = len(img), img.nbytes
    h_reads = L.yakamd_host_alloc(nb)
    assert h_reads
    C.memmove(h_reads, img.ctypes.data, nb)
    t = yak_amd.Table(K, 10, 4, BF)
    for create, again in ((1, True), (0, False)):                      # the benchmark's protocol: create pass, count pass, shrink
        assert L.yakamd_pass_begin(t.h, create) == 0 and L.yakamd_feed_bases_host(t.h, h_reads, nb, 0) == 0, yak_amd._err()
        n = L.yakamd_pass_end(t.h)
        assert n >= 0, yak_amd._err()
        t.h.contents.tot += n
        if again:
            t.destroy_bf(); t.clear()
    t.shrink(2, 1023)
    L.yakamd_host_free(h_reads)
    res = {"genome": a.genome, "snps": n_snp, "reads": n_reads, "k": K, "bf_shift": BF, "table_keys": int(t.tot), "reps": a.reps}

    def stat(xs):
        return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}

    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        fa, out = os.path.join(d, "reads.fa"), os.path.join(tmp, "out.txt")
        with open(fa, "wb") as f:
            f.write(b"".join(b">%d\n%s" % (i, r) for i, r in enumerate(img.tobytes().splitlines(True))))
        del img
        if a.keep:
            with open(os.path.join(d, "table.yak"), "wb") as f:
                f.write(t.dump_bytes())
        ao = allele.AloptT()
        AL.yakamd_alopt_init(C.byref(ao))
        ao.stats_only = 1
        po = phase.PhoptT()
        PHL.yakamd_phopt_init(C.byref(po))
        po.stats_only = 1
        runs = {"alleles": [], "phase": []}
        parts = {"alleles_path": [], "alleles": [], "phase_path": [], "phase": []}
        for i in range(a.reps + 1):                                    # the first round warms
            t0 = time.perf_counter()
            assert AL.yakamd_alleles(C.byref(ao), t.h, fa.encode(), b"/dev/null") == 0, allele._err()
            t1 = time.perf_counter()
            ap_ms, a_ms = path.ms(), allele.ms()
            assert PHL.yakamd_phase(C.byref(po), t.h, fa.encode(), out.encode()) == 0, phase._err()
            t2 = time.perf_counter()
            pp_ms, p_ms = path.ms(), phase.ms()
            if i:
                runs["alleles"].append((t1 - t0) * 1e3); runs["phase"].append((t2 - t1) * 1e3)
                parts["alleles_path"].append(ap_ms); parts["alleles"].append(a_ms); parts["phase_path"].append(pp_ms); parts["phase"].append(p_ms)
        res["tail"] = open(out).read().splitlines()[-1].split("\t")
        said = verbose_line(lambda: PHL.yakamd_phase(C.byref(po), t.h, fa.encode(), b"/dev/null"))
        m = re.search(r"phase: .* (\d+) rounds, the table grew (\d+) times to (\d+) slots", said)
        res["n_round"], res["n_grow"], res["capacity"] = (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else (None, None, None)
    t.close()
    res["end_to_end"] = {k: stat(v) for k, v in runs.items()}
    res["path_ms_in_alleles"] = {p: stat([x[j] for x in parts["alleles_path"]]) for j, p in enumerate(PATH_PARTS)}
    res["path_ms_in_phase"] = {p: stat([x[j] for x in parts["phase_path"]]) for j, p in enumerate(PATH_PARTS)}
    res["allele_ms"] = {p: stat([x[j] for x in parts["alleles"]]) for j, p in enumerate(ALLELE_PARTS)}
    res["phase_ms"] = {p: stat([x[j] for x in parts["phase"]]) for j, p in enumerate(PHASE_PARTS)}
    pm, hm = res["path_ms_in_phase"], res["phase_ms"]
    yard = pm["hits"]["median_ms"] + pm["count_and_scan"]["median_ms"] + pm["emit"]["median_ms"]
    own = hm["compaction"]["median_ms"] + hm["votes_and_growth"]["median_ms"] + hm["solve"]["median_ms"]
    res["yardstick_ms"], res["own_ms"], res["own_over_yardstick"] = round(yard, 3), round(own, 3), round(own / yard, 4) if yard else None
    print(json.dumps(res))
    if a.out:
        tl = res["tail"]
        with open(a.out, "a") as f:
            f.write("a genome of %d bases and a copy with %d SNPs 60 to 90 bases apart; %d error-free %d bp reads (%d-fold per haplotype) counted at k = %d, -b%d, two passes: %d stored keys; "
                    "stats_only, one process, %d rounds behind a warming one.\n" % (a.genome, n_snp, n_reads, READ_LEN, a.cov, K, BF, res["table_keys"], a.reps))
            f.write("T line of yakamd_phase: %s sequences, %s bases, %s paths, %s steps, %s observations (%s full), %s votes on %s pairs, %s bubbles (het %s), %s edges (%s forest, %s discordant), "
                    "%s blocks of two or more, %s bubbles alone, the largest block %s\n" % tuple(tl[1:17]))
            f.write("the solve took %s rounds; the pair table grew %s times to %s slots\n" % (res["n_round"], res["n_grow"], res["capacity"]))
            for title, key, names in (("yakamd_path_ms after yakamd_alleles", "path_ms_in_alleles", PATH_PARTS), ("yakamd_allele_ms after yakamd_alleles", "allele_ms", ALLELE_PARTS),
                                      ("yakamd_path_ms after yakamd_phase", "path_ms_in_phase", PATH_PARTS), ("yakamd_phase_ms after yakamd_phase", "phase_ms", PHASE_PARTS)):
                f.write(title + "\n")
                for p in names:
                    v = res[key][p]
                    f.write("  %-16s median %.2f ms (min %.2f, max %.2f)\n" % (p.replace("_", " "), v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write("the path layer's hits and chain in yakamd_phase %.2f ms; the phase kernels (compaction, votes with growth, solve) %.2f ms: %.1f %% of it\n"
                    % (yard, own, 100.0 * own / yard if yard else 0.0))
            e = res["end_to_end"]
            f.write("end to end: yakamd_phase -s median %.1f ms (min %.1f, max %.1f); yakamd_alleles -s %.1f ms (min %.1f, max %.1f)\n\n"
                    % (e["phase"]["median_ms"], e["phase"]["min_ms"], e["phase"]["max_ms"], e["alleles"]["median_ms"], e["alleles"]["min_ms"], e["alleles"]["max_ms"]))


if __name__ == "__main__":
    main()
