"""Independent restatements for the `yak inspect` tests: a .yak reader, the joint spectrum J[c0][c1] of inspect.c:47-62 in numpy (the probe
of htab.c:93-100 on a dict of the second table), and the lines of inspect.c:64-101 printed from J.  No device is needed here."""
import ctypes as C
import struct

import numpy as np

NC = 1024
M54 = (1 << 54) - 1


def read_yak(fn):
    """(k, pre, keys, sub): every stored key in file order and the sub-table it was read from"""
    data = open(fn, "rb").read()
    assert data[:4] == b"YAK\x02", fn
    k, pre, bits = struct.unpack_from("<3I", data, 4)
    assert bits == 10
    pos, keys, sub = 16, [], []
    for i in range(1 << pre):
        _, size = struct.unpack_from("<2I", data, pos)
        pos += 8
        keys.append(np.frombuffer(data, "<u8", size, pos))
        sub.append(np.full(size, i, np.uint64))
        pos += 8 * size
    return k, pre, np.concatenate(keys), np.concatenate(sub)


def probe_hashes(a, ref):
    """the hash inspect probes the second table with: the rebuilt k-mer hash (key >> 10) << pre | i, or the stored key (ref)"""
    _, pre, keys, sub = a
    return keys.copy() if ref else ((keys >> np.uint64(10)) << np.uint64(pre)) | sub


class Lookup:
    """yak_ch_get() of one table, from its file: sub-table h & mask, then (h >> pre) & (2^54 - 1) against key >> 10"""

    def __init__(self, t):
        self.k, self.pre, keys, sub = t
        ids = (sub.astype(object) << 54) | (keys >> np.uint64(10)).astype(object)
        self.d = dict(zip(ids.tolist(), (keys & np.uint64(1023)).astype(np.int64).tolist()))
        self.hist = np.bincount((keys & np.uint64(1023)).astype(np.int64), minlength=NC).astype(np.int64)

    def get(self, h):
        h = np.asarray(h, np.uint64)
        p = (h & np.uint64((1 << self.pre) - 1)).astype(object)
        kid = ((h >> np.uint64(self.pre)) & np.uint64(M54)).astype(object)
        return np.array([self.d.get(x, 0) for x in ((p << 54) | kid).tolist()], np.int64)


def joint(a, b=None, ref=False):
    """J[c0][c1] of inspect.c:56-60 over the tables read by read_yak (b None: c1 = 0)"""
    J = np.zeros((NC, NC), np.int64)
    c0 = (a[2] & np.uint64(1023)).astype(np.int64)
    c1 = Lookup(b).get(probe_hashes(a, ref)) if b is not None else np.zeros(len(c0), np.int64)
    np.add.at(J, (c0, c1), 1)
    return J


def lines(J, hist, two, max_cnt, kmer, qv_solve):
    """inspect.c:64-101 over J; qv_solve(hist, col, kmer, fpr) -> (tot, qv_raw, qv) is the library's yak_qv_solve"""
    out = []
    tot = J.sum(axis=1)
    if two:
        acc = np.cumsum(J[:, ::-1], axis=1)[:, ::-1]                                # acc[i][j] = sum of J[i][j..1023] (read for j >= 1 only)
        acc_tot, acc_cnt = 0, [0] * NC
        for i in range(NC - 1, -1, -1):
            acc_tot += int(tot[i])
            if acc_tot == 0 or tot[i] == 0:
                continue
            s = "SN\t%d\t%d\t%d" % (i, tot[i], hist[i])
            for j in range(1, max_cnt + 1):
                acc_cnt[j] += int(acc[i, j])
                s += "\t%.4f" % (acc_cnt[j] / acc_tot)
            out.append(s + "\n")
        acc = np.cumsum(J[::-1], axis=0)[::-1]                                      # acc[i][j] = sum of J[i..1023][j]
        for i in range(max_cnt, 0, -1):
            if tot[i] == 0:
                continue
            qtot, qraw, qv = qv_solve(hist, acc[i], kmer, 0.00004)
            out.append("QV\t%d\t%d\t%d\t%.3f\t%.3f\n" % (i, qtot, acc[i, 0], qraw, qv))
    else:
        acc_tot = 0
        for i in range(NC - 1, -1, -1):
            acc_tot += int(tot[i])
            if acc_tot == 0:
                continue
            out.append("HS\t%d\t%d\t%d\t%d\n" % (i, hist[i], tot[i], acc_tot))
    return "".join(out).encode()


def qv_solver(L, QstatT):
    def solve(hist, col, kmer, fpr):
        qs = QstatT()
        h = np.ascontiguousarray(hist, np.int64)
        c = np.ascontiguousarray(col, np.int64)
        L.yak_qv_solve(h.ctypes.data_as(C.POINTER(C.c_int64)), c.ctypes.data_as(C.POINTER(C.c_int64)), kmer, fpr, C.byref(qs))
        return qs.tot, qs.qv_raw, qs.qv
    return solve
