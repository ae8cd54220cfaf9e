"""Measure `yak chkerr` and `yak sexchr` on the device: synthesise a genome, count its reads on the device, then print one JSON line with
the device time of each lookup and of each reduction on two layouts of the same bases -- a handful of long contigs and 20 kb records --,
the wall time of `yak-amd chkerr` / `yak-amd sexchr` end to end, and, on the same files, the reference binary at -t16 and the reference's
own caller files on the library (`oracle/_ref/yak_on_amd`, one host yak_ch_get per k-mer), with whether their outputs equal ours after
sorting the lines (at -t16 the reference prints the sequences in a thread-dependent order).

The genome comes from tools/yaksynth.c.  The assembly is two copies of it (~100 Mb): the first at 0.01 % substitutions, the second at
0.1 %, each with a few foreign inserts of 500 bp.  Reads are error-free 150 bp windows of the genome at random starts.  sexchr's three
tables are counted from three disjoint pieces of the genome (chrY, chrX, PAR) and its two haplotypes are the two copies.
Usage: python tools/chkerr_bench.py [--genome 50e6] [--cov 20] [--contigs 2] [--record 20000] [--dir D]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "yak")
YAK_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "yak_on_amd")
from trioeval_bench import genome, parent_fasta, layout, timed       # noqa: E402


def assembly(g, rng):
    import numpy as np
    acgt = np.frombuffer(b"ACGT", np.uint8)
    haps = []
    for rate, seed in ((1e-4, 21), (1e-3, 23)):
        h = g.copy()
        at = np.flatnonzero(rng.random(len(h)) < rate)
        h[at] = acgt[(np.searchsorted(acgt, h[at]) + rng.integers(1, 4, len(at))) & 3]
        ins = genome(500 * 4, seed)
        parts, prev = [], 0
        for j, c in enumerate((0.15, 0.4, 0.65, 0.9)):
            p = int(c * len(h))
            parts += [h[prev:p], ins[j * 500:(j + 1) * 500]]
            prev = p
        haps.append(np.concatenate(parts + [h[prev:]]))
    return haps


def write_fa(fn, names, img, off, ln):
    with open(fn, "wb") as f:
        for nm, p, n in zip(names, off.tolist(), ln.tolist()):
            f.write(b">" + nm + b"\n" + img[p:p + n].tobytes() + b"\n")


def count(fa, out, k, bf):
    t = time.time()
    subprocess.run([CLI, "count", "-k%d" % k] + (["-b%d" % bf] if bf else []) + ["-o", out, fa], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1800)
    return round(time.time() - t, 2)


def sorted_equal(a, b):
    return sorted(open(a, "rb").read().split(b"\n")) == sorted(open(b, "rb").read().split(b"\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=50e6)
    ap.add_argument("--cov", type=float, default=20)
    ap.add_argument("--contigs", type=int, default=2, help="long contigs per copy")
    ap.add_argument("--record", type=int, default=20000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--bf", type=int, default=34)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true", help="skip the reference binary and yak_on_amd")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    rng = np.random.default_rng(1)
    d = a.dir or tempfile.mkdtemp(prefix="chkerr_bench_")
    os.makedirs(d, exist_ok=True)
    G = int(a.genome)
    res = {"genome": G, "read_cov": a.cov, "k": a.k, "count_bf": a.bf}
    try:
        t = time.time()
        g = genome(G, 7)
        parent_fasta(os.path.join(d, "reads.fa"), g, a.cov, rng)
        haps = assembly(g, rng)
        res["asm_bases"] = int(sum(len(h) for h in haps))
        fa = {}
        for tag, cut in (("long", -(-max(len(x) for x in haps) // a.contigs)), ("20kb", a.record)):
            fa[tag] = os.path.join(d, "asm_%s.fa" % tag)
            write_fa(fa[tag], *layout(haps, cut))
        for i, h in enumerate(haps):                               # sexchr's haplotypes: one file per copy, long contigs
            fa["hap%d" % (i + 1)] = os.path.join(d, "hap%d.fa" % (i + 1))
            write_fa(fa["hap%d" % (i + 1)], *layout([h], -(-len(h) // a.contigs)))
        pieces = {"chrY": g[: G // 10], "chrX": g[G // 10: G // 10 * 4], "par": g[G // 10 * 4: G // 10 * 4 + G // 50]}
        for name, s in pieces.items():
            with open(os.path.join(d, name + ".fa"), "wb") as f:
                f.write(b">" + name.encode() + b"\n" + s.tobytes() + b"\n")
        res["s_synth"] = round(time.time() - t, 1)
        tab = os.path.join(d, "reads.yak")
        res["s_count_reads"] = count(os.path.join(d, "reads.fa"), tab, a.k, a.bf)
        sx = [os.path.join(d, n + ".yak") for n in pieces]
        for n, t_ in zip(pieces, sx):
            res["s_count_" + n] = count(os.path.join(d, n + ".fa"), t_, a.k, 0)

        gb = res["asm_bases"] / 1e9
        h_ce = L.yak_ch_restore(tab.encode())
        h_sc = yak_amd.sexchr_table(*sx)
        assert h_ce and h_sc, yak_amd._err()
        for tag, cut in (("long", -(-max(len(x) for x in haps) // a.contigs)), ("20kb", a.record)):
            names, img, off, ln = layout(haps, cut)
            img = np.concatenate((img, np.full(-len(img) % 16, 10, np.uint8)))
            ns = len(ln)
            bufs = [L.yakamd_dev_alloc(x) for x in (len(img), len(img), off.nbytes, ln.nbytes, ns * 32)]
            assert all(bufs), "device allocation failed"
            d_img, d_out, d_off, d_len, d_cnt = bufs
            assert L.yakamd_memcpy_h2d(d_img, img.ctypes.data, len(img)) == 0
            assert L.yakamd_memcpy_h2d(d_off, off.ctypes.data, off.nbytes) == 0 and L.yakamd_memcpy_h2d(d_len, ln.ctypes.data, ln.nbytes) == 0
            tl, tr, sl, sr = [], [], [], []
            n_sk = C.c_int64()
            for _ in range(a.reps):                                # every call returns after a device synchronise
                t = time.perf_counter()
                assert L.yakamd_chkerr_lookup_dev(h_ce, d_img, len(img), 3, d_out) == 0, yak_amd._err()
                tl.append(time.perf_counter() - t)
                d_sk = C.c_void_p()
                t = time.perf_counter()
                assert L.yakamd_chkerr_streaks_dev(5, d_out, d_off, ns, len(img), C.byref(d_sk), C.byref(n_sk), None) == 0, yak_amd._err()
                tr.append(time.perf_counter() - t)
                L.yakamd_dev_free(d_sk.value)
                t = time.perf_counter()
                assert L.yakamd_triobin_lookup_dev(h_sc, d_img, len(img), d_out) == 0, yak_amd._err()
                sl.append(time.perf_counter() - t)
                t = time.perf_counter()
                assert L.yakamd_sexchr_reduce_dev(d_out, d_off, d_len, ns, len(img), d_cnt, None) == 0, yak_amd._err()
                sr.append(time.perf_counter() - t)
            res[tag] = {"records": ns, "chkerr_streaks": n_sk.value,
                        "chkerr": {"ms_lookup": round(min(tl) * 1e3, 3), "ms_reduce": round(min(tr) * 1e3, 3),
                                   "ms_lookup_per_gb": round(min(tl) * 1e3 / gb, 2), "reduce_over_lookup": round(min(tr) / min(tl), 4)},
                        "sexchr": {"ms_lookup": round(min(sl) * 1e3, 3), "ms_reduce": round(min(sr) * 1e3, 3),
                                   "ms_lookup_per_gb": round(min(sl) * 1e3 / gb, 2), "reduce_over_lookup": round(min(sr) / min(sl), 4)}}
            for p in bufs:
                L.yakamd_dev_free(p)
        L.yak_ch_destroy(h_ce)
        L.yak_ch_destroy(h_sc)

        runs = {"chkerr": ([CLI, "chkerr", tab, fa["long"]], [REF, "chkerr", "-t16", tab, fa["long"]],
                           [YAK_ON_AMD, "chkerr", "-t16", tab, fa["long"]]),
                "sexchr": ([CLI, "sexchr"] + sx + [fa["hap1"], fa["hap2"]], [REF, "sexchr", "-t16"] + sx + [fa["hap1"], fa["hap2"]],
                           [YAK_ON_AMD, "sexchr", "-t16"] + sx + [fa["hap1"], fa["hap2"]])}
        for cmd, (mine_cmd, ref_cmd, on_amd_cmd) in runs.items():
            mine = os.path.join(d, cmd + "_gpu.txt")
            e = res["e2e_" + cmd] = {"s_yak_amd": round(timed(mine_cmd, mine, 3600), 2)}
            e["md5_yak_amd"] = hashlib.md5(open(mine, "rb").read()).hexdigest()
            e["lines"] = open(mine, "rb").read().count(b"\n")
            if a.no_ref:
                continue
            for tag, c, exe in (("ref_t16", ref_cmd, REF), ("yak_on_amd_t16", on_amd_cmd, YAK_ON_AMD)):
                if not os.path.exists(exe):
                    e["s_" + tag] = "not built"
                    continue
                theirs = os.path.join(d, "%s_%s.txt" % (cmd, tag))
                e["s_" + tag] = round(timed(c, theirs, 7200), 2)
                e["equal_" + tag] = sorted_equal(mine, theirs)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
