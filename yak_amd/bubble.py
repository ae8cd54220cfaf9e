"""The simple bubbles of the compacted de Bruijn graph of a count table called on the GPU (libyak_amd_bubble.so above libyak_amd_gfa.so,
libyak_amd_walk.so and libyak_amd.so; include/yak_amd_bubble.h): Bubbles(walk, gfa, k) keeps the records of a
yak_amd.walk.Walk and its yak_amd.gfa.Gfa in device memory and hands them out as a numpy array; bubbles() is `yak-amd bubbles` through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.gfa
from yak_amd import ChT, UgoptT, _layer
from yak_amd._layer import P

BUBBLE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_bubble.so")
BUBBLE_H_SYMBOLS = [
    "yakamd_bubble_open", "yakamd_bubble_stats", "yakamd_bubble_records_dev", "yakamd_bubble_close", "yakamd_bubbles", "yakamd_bubble_ms",
    "yakamd_bubble_last_error", "yakamd_bubble_tally_names", "yakamd_bubble_tally_read", "yakamd_bubble_tally_reset",
]
TYPES = "SEI"                                  # YAKAMD_BUBBLE_S, _E, _I
NO_HD = (1 << 64) - 1                          # hd of arms of two lengths


class BubbleT(C.Structure):                    # yakamd_bubble_t, include/yak_amd_bubble.h
    _fields_ = [("src", C.c_uint64), ("sink", C.c_uint64), ("arm", C.c_uint64 * 2), ("n_node", C.c_uint64 * 2), ("kc", C.c_uint64 * 2), ("hd", C.c_uint64),
                ("type", C.c_uint64)]


class BubstatT(C.Structure):                   # yakamd_bubstat_t
    _fields_ = [("n_bubble", C.c_uint64), ("n_type", C.c_uint64 * 3), ("n_tip", C.c_uint64), ("tip_nodes", C.c_uint64), ("max_arm_nodes", C.c_uint64),
                ("n_fork", C.c_uint64)]


_lib = None


def lib():
    """Load libyak_amd_bubble.so (once), after the three libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        _lib = _layer.load(BUBBLE_LIB_PATH, yak_amd.gfa.lib, {
            **_layer.common("bubble"),
            "yakamd_bubble_open": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int]), "yakamd_bubble_stats": (C.c_int, [C.c_void_p, P(BubstatT)]),
            "yakamd_bubble_records_dev": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]), "yakamd_bubble_close": (None, [C.c_void_p]),
            "yakamd_bubbles": (C.c_int, [P(UgoptT), P(ChT), C.c_char_p]), "yakamd_bubble_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "bubble")


def tally():
    """{kernel instantiation: launches since the last yakamd_bubble_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "bubble")


def ms():
    """the milliseconds of the calling thread's last open or command: copies, first links, find, classify, text"""
    out = (C.c_double * 5)()
    lib().yakamd_bubble_ms(out)
    return list(out)


class Bubbles:
    """the simple bubbles of a device walk (a yak_amd.walk.Walk) and its links (a yak_amd.gfa.Gfa) at the table's k: yakamd_bubble_open ...
    yakamd_bubble_close.  Copies are taken at the open: the records outlive the walk and the links"""

    def __init__(self, walk, gfa, k):
        self.L, self.M = lib(), yak_amd.lib()
        self.b = self.L.yakamd_bubble_open(walk.w if walk is not None else None, gfa.g if gfa is not None else None, k)
        if not self.b:
            raise RuntimeError("yakamd_bubble_open failed: " + _err())

    def close(self):
        if self.b:
            self.L.yakamd_bubble_close(self.b)
            self.b = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = BubstatT()
        if self.L.yakamd_bubble_stats(self.b, C.byref(st)) != 0:
            raise RuntimeError("yakamd_bubble_stats failed: " + _err())
        return dict(n_bubble=int(st.n_bubble), n_type=[int(v) for v in st.n_type], n_tip=int(st.n_tip), tip_nodes=int(st.tip_nodes),
                    max_arm_nodes=int(st.max_arm_nodes), n_fork=int(st.n_fork))

    def records(self):
        """the bubbles in list order (by src): src, sink, arm[2], each unitig << 1 | (1 for '-'); n_node[2] and kc[2] of the arms; hd (NO_HD for arms
        of two lengths); type, an index into TYPES.  Through device memory of the caller's, as Gfa.links() gets its entries"""
        import numpy as np
        dtype = np.dtype([("src", "<u8"), ("sink", "<u8"), ("arm", "<u8", 2), ("n_node", "<u8", 2), ("kc", "<u8", 2), ("hd", "<u8"), ("type", "<u8")])
        n = self.L.yakamd_bubble_records_dev(self.b, None, 0)
        if n < 0:
            raise RuntimeError("the size query failed: " + _err())
        out = np.zeros(n, dtype)
        if n == 0:
            return out
        d = self.M.yakamd_dev_alloc(n * 80)
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + yak_amd._err())
        try:
            if self.L.yakamd_bubble_records_dev(self.b, d, n) != n:
                raise RuntimeError("the copy failed: " + _err())
            if self.M.yakamd_memcpy_d2h(out.ctypes.data, d, n * 80) != 0:
                raise RuntimeError(yak_amd._err())
        finally:
            self.M.yakamd_dev_free(d)
        return out


def bubbles(table_yak, min_cnt=1, stats_only=False):
    """`yak-amd bubbles` through the C ABI (yak_ch_restore + yakamd_bubbles): the B lines, or with stats_only the text of `unitigs -G -s` and
    the B line of the tallies"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = UgoptT()
        M.yakamd_ugopt_init(C.byref(o))
        o.min_cnt, o.stats_only = min_cnt, int(bool(stats_only))
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "bubbles.txt")
            if L.yakamd_bubbles(C.byref(o), h, out.encode()) != 0:
                raise RuntimeError("yakamd_bubbles failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
