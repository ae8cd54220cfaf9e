"""What `yak print` writes, restated in Python (reference main.c:302-320 on htab.c:353-367), and the oracle's getseq behind it: the
checker of tests/test_tablecmds.py and tests/test_gpu_tablecmds.py."""
import ctypes as C
import struct

M64 = (1 << 64) - 1


def hash64_inv(x, m):
    """reference yak-priv.h:41-68"""
    t = (x - (x << 31)) & M64; x = (x - (t << 31)) & m
    t = x ^ x >> 28; x = x ^ t >> 28
    x = (x * 14933078535860113213) & m
    t = x ^ x >> 14; t = x ^ t >> 14; t = x ^ t >> 14; x = x ^ t >> 14
    x = (x * 15244667743933553977) & m
    t = x ^ x >> 24; x = x ^ t >> 24
    t = ~x & M64; t = ~(x - (t << 21)) & M64; t = ~(x - (t << 21)) & M64; x = ~(x - (t << 21)) & m
    return x


def lines(pairs, k, counts):
    """the bytes of main.c:308-317 for (x, c) pairs"""
    out = []
    for x, c in pairs:
        s = "".join("ACGT"[x >> 2 * j & 3] for j in range(k - 1, -1, -1))
        out.append(s + ("\t%d\n" % c if counts else "\n"))
    return "".join(out).encode()


def read_yak(fn):
    """(k, pre, [keys of sub-table 0, 1, ...]) of a .yak file (htab.c:373-394)"""
    d = open(fn, "rb").read()
    assert d[:4] == b"YAK\2"
    k, pre, _ = struct.unpack_from("<3I", d, 4)
    at, subs = 16, []
    for _ in range(1 << pre):
        _, n = struct.unpack_from("<2I", d, at)
        subs.append(list(struct.unpack_from("<%dQ" % n, d, at + 8)))
        at += 8 + 8 * n
    return k, pre, subs


def file_order_pairs(fn):
    """(x, c) of every key in the order the file stores them: what print would list if nothing moved a key after the load"""
    k, pre, subs = read_yak(fn)
    m = (1 << 2 * k) - 1
    return k, [(hash64_inv((key >> 10) << pre | w, m), key & 1023) for w, keys in enumerate(subs) for key in keys]


class Knt(C.Structure):                        # yko_knt_t, oracle/yko.h
    _fields_ = [("x", C.c_uint64), ("c", C.c_int)]


def oracle_getseq(oracle, h, lo=0, hi=None):
    """(x, c) of sub-tables [lo, hi) of an oracle table, by yko_ch_getseq"""
    O = oracle.lib()
    O.yko_ch_getseq.restype = C.POINTER(Knt)
    O.yko_ch_getseq.argtypes = [C.POINTER(oracle.Ch), C.c_int, C.POINTER(C.c_uint32)]
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    out = []
    for w in range(lo, (1 << h.contents.pre) if hi is None else hi):
        n = C.c_uint32()
        a = O.yko_ch_getseq(h, w, C.byref(n))
        out += [(a[j].x, a[j].c) for j in range(n.value)]
        free(C.cast(a, C.c_void_p))
    return out


def oracle_print(oracle, fn, counts, tighten=True):
    """the oracle's restore, tighten and getseq over all sub-tables, formatted: what the reference's `print [-c] fn` writes"""
    O = oracle.lib()
    h = O.yko_ch_restore(fn.encode())
    assert h
    try:
        if tighten:
            O.yko_ch_tighten(h)
        return lines(oracle_getseq(oracle, h), h.contents.k, counts)
    finally:
        O.yko_ch_destroy(h)
