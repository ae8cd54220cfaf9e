"""Measure `yak inspect` on the device: synthesise a read set and an assembly of one genome with tools/yaksynth, count both on the device,
then print one JSON line with the device time of the table join (in1 = the reads' table, tens of millions of keys, against in2 = the
assembly's) and its rate in G probes/s, the one-table (HS) tally, the wall time of `yak-amd inspect` end to end split into in2's restore,
in1's file read and the join (the library's own [M::yakamd_inspect] line), and -- if oracle/_ref/yak exists -- the reference binary's
`inspect` on the same files and whether `yak-amd inspect -R` wrote the same bytes.

Usage: python tools/inspect_bench.py [--genome 10e6] [--cov 20] [--err 0.005] [--k 31] [--reps 5] [--dir D]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "yak")
SYNTH = os.path.join(ROOT, "tools", "yaksynth")


def timed(cmd, out_fn, timeout):
    t = time.time()
    with open(out_fn, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return time.time() - t, r.stderr.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=10e6)
    ap.add_argument("--cov", type=float, default=20)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import yak_amd
    L = yak_amd.lib()
    d = a.dir or tempfile.mkdtemp(prefix="inspect_bench_")
    os.makedirs(d, exist_ok=True)
    G = int(a.genome)
    res = {"genome": G, "cov": a.cov, "err": a.err, "k": a.k}
    try:
        t = time.time()
        reads, asm = os.path.join(d, "reads.fa"), os.path.join(d, "asm.fa")
        n_reads = int(a.cov * G / 150)
        subprocess.run([SYNTH, "-a", "-n", str(n_reads), "-l", "150", "-g", str(G), "-s", "5", "-e", str(a.err), "-N", "0", "-o", reads], check=True)
        subprocess.run([SYNTH, "-T", "-n", "10", "-l", str(G // 10), "-s", "5", "-o", asm], check=True)
        res["s_synth"] = round(time.time() - t, 1)
        tabs = {}
        for who, fa in (("reads", reads), ("asm", asm)):
            tabs[who] = os.path.join(d, who + ".yak")
            t = time.time()
            subprocess.run([CLI, "count", "-k%d" % a.k, "-o", tabs[who], fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1800)
            res["s_count_" + who] = round(time.time() - t, 2)

        # the join alone: in1's keys (file order, headers stripped) resident, in2 restored
        raw = np.fromfile(tabs["reads"], np.uint8)
        k, pre = (int(x) for x in raw[4:12].view(np.uint32))
        words = raw[16:].view(np.uint64)
        keys, off, pos = [], [0], 0
        for i in range(1 << pre):
            size = int(words[pos] >> np.uint64(32))
            keys.append(words[pos + 1:pos + 1 + size])
            off.append(off[-1] + size)
            pos += 1 + size
        keys = np.ascontiguousarray(np.concatenate(keys))
        off = np.array(off, np.uint64)
        n = len(keys)
        res["in1_keys"] = n
        d_keys, d_off, d_J = L.yakamd_dev_alloc(keys.nbytes), L.yakamd_dev_alloc(off.nbytes), L.yakamd_dev_alloc(8 << 20)
        assert d_keys and d_off and d_J, "device allocation failed"
        assert L.yakamd_memcpy_h2d(d_keys, keys.ctypes.data, keys.nbytes) == 0 and L.yakamd_memcpy_h2d(d_off, off.ctypes.data, off.nbytes) == 0
        b = L.yak_ch_restore(tabs["asm"].encode())
        assert b, yak_amd._err()
        hist = np.zeros(1024, np.int64)
        L.yak_ch_hist(b, hist.ctypes.data_as(C.POINTER(C.c_int64)), 1)
        res["in2_keys"] = int(hist.sum())
        zero = np.zeros(1 << 20, np.uint64)
        times = {}
        for tag, h, ref in (("join", b, 0), ("join_ref_probe", b, 1), ("hs_only", None, 0)):
            ts = []
            for _ in range(a.reps):
                assert L.yakamd_memcpy_h2d(d_J, zero.ctypes.data, zero.nbytes) == 0
                assert L.yakamd_device_sync() == 0
                t = time.perf_counter()
                assert L.yakamd_inspect_dev(h, k, pre, 0, 1 << pre, d_keys, n, d_off, 0, ref, d_J, None) == 0, yak_amd._err()
                ts.append(time.perf_counter() - t)
            times[tag] = min(ts)
            if tag == "join":
                J = np.zeros(1 << 20, np.uint64)
                assert L.yakamd_memcpy_d2h(J.ctypes.data, d_J, J.nbytes) == 0
        res["ms_join"] = round(times["join"] * 1e3, 3)
        res["g_probes_per_s"] = round(n / times["join"] / 1e9, 2)
        res["ms_join_ref_probe"] = round(times["join_ref_probe"] * 1e3, 3)
        res["ms_hs_only"] = round(times["hs_only"] * 1e3, 3)
        res["hs_only_g_keys_per_s"] = round(n / times["hs_only"] / 1e9, 2)
        L.yak_ch_destroy(b)
        for p in (d_keys, d_off, d_J):
            L.yakamd_dev_free(p)

        mine = os.path.join(d, "out_gpu.txt")
        s, err = timed([CLI, "inspect", tabs["reads"], tabs["asm"]], mine, 3600)
        res["s_e2e_yak_amd"] = round(s, 3)
        m = re.search(r"restore ([0-9.]+) s, read ([0-9.]+) s, join ([0-9.]+) s", err)
        if m:
            res["s_e2e_restore"], res["s_e2e_read"], res["s_e2e_join"] = (float(x) for x in m.groups())
        res["s_e2e_hs_yak_amd"] = round(timed([CLI, "inspect", tabs["reads"]], os.path.join(d, "hs_gpu.txt"), 3600)[0], 3)
        mine_r = os.path.join(d, "out_gpu_R.txt")
        res["s_e2e_yak_amd_R"] = round(timed([CLI, "inspect", "-R", tabs["reads"], tabs["asm"]], mine_r, 3600)[0], 3)
        if os.path.exists(REF):
            theirs = os.path.join(d, "out_ref.txt")
            res["s_e2e_ref"] = round(timed([REF, "inspect", tabs["reads"], tabs["asm"]], theirs, 7200)[0], 3)
            res["R_equals_ref"] = open(mine_r, "rb").read() == open(theirs, "rb").read()
            theirs_hs = os.path.join(d, "hs_ref.txt")
            res["s_e2e_hs_ref"] = round(timed([REF, "inspect", tabs["reads"]], theirs_hs, 7200)[0], 3)
            res["hs_equals_ref"] = open(os.path.join(d, "hs_gpu.txt"), "rb").read() == open(theirs_hs, "rb").read()
        tot = J.reshape(1024, 1024).sum(axis=1)
        res["in1_keys_found_in_in2"] = int(J.reshape(1024, 1024)[:, 1:].sum())
        res["in1_keys_check"] = int(tot.sum()) == n
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
