"""Measure `yak trioeval` on the device: synthesise a diploid, count the parents on the device, then print one JSON line with
the device time of the flag lookup and of the streak reduction on two layouts of the same bases -- a handful of long contigs and
20 kb records -- (per Gb too), the wall time of `yak-amd trioeval` end to end, the reference binary's `trioeval -t16` on the same
files (if oracle/_ref/yak exists) and whether the two outputs are equal after sorting their lines (the reference's F lines at -t16
are not in input order).

The base genome comes from tools/yaksynth.c; the paternal haplotype is it with a few insertions of its own, the maternal one is it
at ~0.1 % SNPs with insertions of its own.  Parent reads are error-free 150 bp windows at random starts.
Usage: python tools/trioeval_bench.py [--genome 50e6] [--cov 15] [--snp 0.001] [--contigs 2] [--record 20000] [--dir D]
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
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "yak")


def genome(n, seed):
    import numpy as np
    L = C.CDLL(os.path.join(ROOT, "tools", "libyaksynth.so"))
    L.yaksynth_genome.argtypes = [C.c_void_p, C.c_int64, C.c_uint64]
    g = np.empty(n, np.uint8)
    L.yaksynth_genome(g.ctypes.data, n, seed)
    return g


def haplotypes(n, snp, rng):
    import numpy as np
    base = genome(n, 7)
    core = base.copy()
    at = np.flatnonzero(rng.random(n) < snp)
    core[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), core[at]) + rng.integers(1, 4, len(at))) & 3]
    haps = []
    for h, seed, cuts in ((base, 11, (0.2, 0.45, 0.7)), (core, 13, (0.3, 0.6, 0.85))):
        ins = genome(20000 * len(cuts), seed)
        parts, prev = [], 0
        for j, c in enumerate(cuts):
            p = int(c * n)
            parts += [h[prev:p], ins[j * 20000:(j + 1) * 20000]]
            prev = p
        haps.append(np.concatenate(parts + [h[prev:]]))
    return haps


def parent_fasta(fn, hap, cov, rng):
    import numpy as np
    n = int(cov * len(hap) / 150)
    st = rng.integers(0, len(hap) - 150, n)
    win = np.lib.stride_tricks.sliding_window_view(hap, 150)
    with open(fn, "wb") as f:
        for b in range(0, n, 1 << 20):
            s = win[st[b:b + (1 << 20)]]
            rec = np.empty((len(s), 153), np.uint8)
            rec[:, 0], rec[:, 1], rec[:, 2:152], rec[:, 152] = ord(">"), ord("\n"), s, ord("\n")
            f.write(rec.tobytes())


def layout(haps, cut):
    """records of `cut` bases (the last one of a haplotype shorter): names, image (each record + '\\n'), off, len"""
    import numpy as np
    names, seqs = [], []
    for hi, h in enumerate(haps):
        for j, p in enumerate(range(0, len(h), cut)):
            names.append(b"h%d_%d" % (hi + 1, j))
            seqs.append(h[p:p + cut])
    ln = np.array([len(s) for s in seqs], np.uint32)
    off = np.concatenate(([0], np.cumsum(ln.astype(np.uint64) + 1)[:-1])).astype(np.uint64)
    nl = np.array([10], np.uint8)
    img = np.concatenate([x for s in seqs for x in (s, nl)])
    return names, img, off, ln


def timed(cmd, out_fn, timeout):
    t = time.time()
    with open(out_fn, "wb") as f:
        subprocess.run(cmd, check=True, stdout=f, stderr=subprocess.DEVNULL, timeout=timeout)
    return time.time() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=50e6)
    ap.add_argument("--cov", type=float, default=15)
    ap.add_argument("--snp", type=float, default=0.001)
    ap.add_argument("--contigs", type=int, default=2, help="long contigs per haplotype")
    ap.add_argument("--record", type=int, default=20000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--bf", type=int, default=34)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    rng = np.random.default_rng(1)
    d = a.dir or tempfile.mkdtemp(prefix="trioeval_bench_")
    os.makedirs(d, exist_ok=True)
    G = int(a.genome)
    res = {"genome": G, "snp": a.snp, "parent_cov": a.cov, "k": a.k}
    try:
        t = time.time()
        haps = haplotypes(G, a.snp, rng)
        for who, h in zip(("pat", "mat"), haps):
            parent_fasta(os.path.join(d, who + ".fa"), h, a.cov, rng)
        res["asm_bases"] = int(sum(len(h) for h in haps))
        res["s_synth"] = round(time.time() - t, 1)
        tabs = {}
        for who in ("pat", "mat"):
            tabs[who] = os.path.join(d, who + ".yak")
            t = time.time()
            subprocess.run([CLI, "count", "-k%d" % a.k, "-b%d" % a.bf, "-o", tabs[who], os.path.join(d, who + ".fa")], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1800)
            res["s_count_" + who] = round(time.time() - t, 2)

        h = yak_amd.triobin_table(tabs["pat"], tabs["mat"])
        gb = res["asm_bases"] / 1e9
        long_fa = None
        for tag, cut in (("long", -(-max(len(x) for x in haps) // a.contigs)), ("20kb", a.record)):
            names, img, off, ln = layout(haps, cut)
            if tag == "long":
                long_fa = os.path.join(d, "asm_long.fa")
                with open(long_fa, "wb") as f:
                    for nm, p, n in zip(names, off.tolist(), ln.tolist()):
                        f.write(b">" + nm + b"\n" + img[p:p + n].tobytes() + b"\n")
            img = np.concatenate((img, np.full(-len(img) % 16, 10, np.uint8)))
            ns = len(ln)
            bufs = [L.yakamd_dev_alloc(x) for x in (len(img), len(img), off.nbytes, ln.nbytes, ns * 24)]
            assert all(bufs), "device allocation failed"
            d_img, d_flag, d_off, d_len, d_cnt = bufs
            assert L.yakamd_memcpy_h2d(d_img, img.ctypes.data, len(img)) == 0
            assert L.yakamd_memcpy_h2d(d_off, off.ctypes.data, off.nbytes) == 0 and L.yakamd_memcpy_h2d(d_len, ln.ctypes.data, ln.nbytes) == 0
            tl, tr, trl = [], [], []
            n_sk = C.c_int64()
            for _ in range(a.reps):
                t = time.perf_counter()
                assert L.yakamd_triobin_lookup_dev(h, d_img, len(img), d_flag) == 0, yak_amd._err()
                tl.append(time.perf_counter() - t)
                t = time.perf_counter()
                assert L.yakamd_trioeval_reduce_dev(a.k, 2, d_flag, d_off, d_len, ns, len(img), d_cnt, None, C.byref(n_sk), None) == 0, yak_amd._err()
                tr.append(time.perf_counter() - t)
                d_sk = C.c_void_p()
                t = time.perf_counter()
                assert L.yakamd_trioeval_reduce_dev(a.k, 2, d_flag, d_off, d_len, ns, len(img), d_cnt, C.byref(d_sk), C.byref(n_sk), None) == 0
                trl.append(time.perf_counter() - t)
                L.yakamd_dev_free(d_sk.value)
            res[tag] = {"records": ns, "streaks": n_sk.value, "ms_lookup": round(min(tl) * 1e3, 3), "ms_reduce": round(min(tr) * 1e3, 3),
                        "ms_reduce_with_list": round(min(trl) * 1e3, 3), "ms_lookup_per_gb": round(min(tl) * 1e3 / gb, 2),
                        "ms_reduce_per_gb": round(min(tr) * 1e3 / gb, 2)}
            res[tag]["reduce_over_lookup"] = round(min(tr) / min(tl), 4)
            for p in bufs:
                L.yakamd_dev_free(p)
        res["reduce_long_over_20kb"] = round(res["long"]["ms_reduce"] / res["20kb"]["ms_reduce"], 3)
        L.yak_ch_destroy(h)

        mine = os.path.join(d, "out_gpu.txt")
        res["s_e2e_yak_amd"] = round(timed([CLI, "trioeval", tabs["pat"], tabs["mat"], long_fa], mine, 3600), 2)
        res["md5_yak_amd"] = hashlib.md5(open(mine, "rb").read()).hexdigest()
        if os.path.exists(REF):
            theirs = os.path.join(d, "out_ref.txt")
            res["s_e2e_ref_t16"] = round(timed([REF, "trioeval", "-t16", tabs["pat"], tabs["mat"], long_fa], theirs, 7200), 2)
            res["outputs_equal"] = sorted(open(mine, "rb").read().split(b"\n")) == sorted(open(theirs, "rb").read().split(b"\n"))
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
