"""Measure `yak triobin` on the device: synthesise a trio, count the parents on the device, then print one JSON line
with the device time of the flag lookup and of the per-read reduction (per Gb of child bases), the wall time of
`yak-amd triobin` end to end, the reference binary's `triobin -t32` on the same files (if oracle/_ref/yak exists) and
whether the two outputs are equal.

The parents are two unrelated random genomes (tools/yaksynth.c, one seed each) read at 150 bp; the child's reads come
half from each.  Usage: python tools/triobin_bench.py [--genome 50e6] [--cov 30] [--child 1e9] [--read 15000] [--dir D]
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


def reads(n, length, genome, seed, err):
    from __graft_entry__ import _synth
    return _synth(n, length, genome, seed, err=err, nrate=0.0)


def write_fasta(fn, image, names=None):
    seqs = image.rstrip(b"\n").split(b"\n")
    if names is None:
        data = b">\n" + image.rstrip(b"\n").replace(b"\n", b"\n>\n") + b"\n"
    else:
        data = b"".join(b">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))
    with open(fn, "wb") as f:
        f.write(data)
    return len(seqs)


def timed(cmd, out_fn, timeout):
    t = time.time()
    with open(out_fn, "wb") as f:
        subprocess.run(cmd, check=True, stdout=f, stderr=subprocess.DEVNULL, timeout=timeout)
    return time.time() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=50e6)
    ap.add_argument("--cov", type=float, default=30)
    ap.add_argument("--child", type=float, default=1e9)
    ap.add_argument("--read", type=int, default=15000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--bf", type=int, default=34)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    d = a.dir or tempfile.mkdtemp(prefix="triobin_bench_")
    os.makedirs(d, exist_ok=True)
    G = int(a.genome)
    res = {"genome": G, "parent_cov": a.cov, "child_bases": 0, "read_len": a.read, "k": a.k}
    try:
        t = time.time()
        n_par = int(a.cov * G / 150)
        for who, seed in (("pat", 101), ("mat", 202)):
            write_fasta(os.path.join(d, who + ".fa"), reads(n_par, 150, G, seed, 0.002))
        n_child = int(a.child / a.read)
        img = reads(n_child // 2, a.read, G, 101, 0.001) + reads(n_child - n_child // 2, a.read, G, 202, 0.001)
        child = os.path.join(d, "child.fa")
        write_fasta(child, img, [b"c%d" % i for i in range(n_child)])
        res["child_bases"] = n_child * a.read
        res["s_synth"] = round(time.time() - t, 1)
        tabs = {}
        for who in ("pat", "mat"):
            tabs[who] = os.path.join(d, who + ".yak")
            t = time.time()
            subprocess.run([CLI, "count", "-k%d" % a.k, "-b%d" % a.bf, "-o", tabs[who], os.path.join(d, who + ".fa")], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1800)
            res["s_count_" + who] = round(time.time() - t, 2)

        # device time of the two kernels on the whole child image (one batch), best of --reps
        h = yak_amd.triobin_table(tabs["pat"], tabs["mat"])
        img = bytes(img) + b"\n" * (-len(img) % 16)
        arr = np.frombuffer(img, np.uint8)
        off = np.arange(n_child, dtype=np.uint64) * (a.read + 1)
        ln = np.full(n_child, a.read, np.uint32)
        d_img, d_flag = L.yakamd_dev_alloc(len(img)), L.yakamd_dev_alloc(len(img))
        d_off, d_len, d_cnt = L.yakamd_dev_alloc(off.nbytes), L.yakamd_dev_alloc(ln.nbytes), L.yakamd_dev_alloc(n_child * 76)
        assert all((d_img, d_flag, d_off, d_len, d_cnt)), "device allocation failed"
        assert L.yakamd_memcpy_h2d(d_img, arr.ctypes.data, len(img)) == 0
        assert L.yakamd_memcpy_h2d(d_off, off.ctypes.data, off.nbytes) == 0 and L.yakamd_memcpy_h2d(d_len, ln.ctypes.data, ln.nbytes) == 0
        tl, tr = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            assert L.yakamd_triobin_lookup_dev(h, d_img, len(img), d_flag) == 0, yak_amd._err()
            tl.append(time.perf_counter() - t)
            t = time.perf_counter()
            assert L.yakamd_triobin_reduce_dev(a.k, d_flag, d_off, d_len, n_child, d_cnt, None) == 0, yak_amd._err()
            tr.append(time.perf_counter() - t)
        gb = res["child_bases"] / 1e9
        res["ms_lookup"] = round(min(tl) * 1e3, 2)
        res["ms_reduce"] = round(min(tr) * 1e3, 2)
        res["ms_lookup_per_gb"] = round(min(tl) * 1e3 / gb, 2)
        res["ms_reduce_per_gb"] = round(min(tr) * 1e3 / gb, 2)
        res["g_probes_per_s"] = round(res["child_bases"] / min(tl) / 1e9, 1)
        for p in (d_img, d_flag, d_off, d_len, d_cnt):
            L.yakamd_dev_free(p)
        L.yak_ch_destroy(h)

        mine = os.path.join(d, "out_gpu.txt")
        res["s_e2e_yak_amd"] = round(timed([CLI, "triobin", tabs["pat"], tabs["mat"], child], mine, 3600), 2)
        res["md5_yak_amd"] = hashlib.md5(open(mine, "rb").read()).hexdigest()
        if os.path.exists(REF):
            theirs = os.path.join(d, "out_ref.txt")
            res["s_e2e_ref_t32"] = round(timed([REF, "triobin", "-t32", tabs["pat"], tabs["mat"], child], theirs, 7200), 2)
            res["outputs_equal"] = open(mine, "rb").read() == open(theirs, "rb").read()
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
