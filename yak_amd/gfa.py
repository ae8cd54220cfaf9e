"""The links between the unitigs of a count table's de Bruijn graph made on the GPU, and the graph as GFA 1 (libyak_amd_gfa.so beside
libyak_amd_walk.so and libyak_amd.so; include/yak_amd_gfa.h): Gfa(walk, k) keeps the links of a yak_amd.walk.Walk in device
memory and hands them out as a numpy array; gfa() is `yak-amd unitigs -G` through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.walk
from yak_amd import ChT, UgoptT, _layer
from yak_amd._layer import P

GFA_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_gfa.so")
GFA_H_SYMBOLS = [
    "yakamd_gfa_open", "yakamd_gfa_stats", "yakamd_gfa_links_dev", "yakamd_gfa_close", "yakamd_unitigs_gfa", "yakamd_gfa_ms", "yakamd_gfa_last_error",
    "yakamd_gfa_tally_names", "yakamd_gfa_tally_read", "yakamd_gfa_tally_reset",
]


class GfastatT(C.Structure):                   # yakamd_gfastat_t, include/yak_amd_gfa.h
    _fields_ = [("n_unitig", C.c_uint64), ("n_open", C.c_uint64), ("n_cycle", C.c_uint64), ("n_link", C.c_uint64), ("end_deg", C.c_uint64 * 5),
                ("table_slots", C.c_uint64), ("max_probe", C.c_uint64)]


_lib = None


def lib():
    """Load libyak_amd_gfa.so (once), after the two libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        _lib = _layer.load(GFA_LIB_PATH, yak_amd.walk.lib, {
            **_layer.common("gfa"),
            "yakamd_gfa_open": (C.c_void_p, [C.c_void_p, C.c_int]), "yakamd_gfa_stats": (C.c_int, [C.c_void_p, P(GfastatT)]),
            "yakamd_gfa_links_dev": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]), "yakamd_gfa_close": (None, [C.c_void_p]),
            "yakamd_unitigs_gfa": (C.c_int, [P(UgoptT), P(ChT), C.c_char_p]), "yakamd_gfa_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "gfa")


def tally():
    """{kernel instantiation: launches since the last yakamd_gfa_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "gfa")


class Gfa:
    """the links of a device walk (a yak_amd.walk.Walk) at its table's k: yakamd_gfa_open ... yakamd_gfa_close"""

    def __init__(self, walk, k):
        self.L, self.M = lib(), yak_amd.lib()
        self.g = self.L.yakamd_gfa_open(walk.w if walk is not None else None, k)
        if not self.g:
            raise RuntimeError("yakamd_gfa_open failed: " + _err())

    def close(self):
        if self.g:
            self.L.yakamd_gfa_close(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = GfastatT()
        if self.L.yakamd_gfa_stats(self.g, C.byref(st)) != 0:
            raise RuntimeError("yakamd_gfa_stats failed: " + _err())
        return dict(n_unitig=int(st.n_unitig), n_open=int(st.n_open), n_cycle=int(st.n_cycle), n_link=int(st.n_link), end_deg=[int(v) for v in st.end_deg],
                    table_slots=int(st.table_slots), max_probe=int(st.max_probe))

    def links(self):
        """the links in list order: (from, to), each unitig << 1 | (1 for '-'); through device memory of the caller's, as Walk.map() gets its entries"""
        import numpy as np
        dtype = np.dtype([("from", "<u8"), ("to", "<u8")])
        n = self.L.yakamd_gfa_links_dev(self.g, None, 0)
        if n < 0:
            raise RuntimeError("the size query failed: " + _err())
        out = np.zeros(n, dtype)
        if n == 0:
            return out
        d = self.M.yakamd_dev_alloc(n * 16)
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + yak_amd._err())
        try:
            if self.L.yakamd_gfa_links_dev(self.g, d, n) != n:
                raise RuntimeError("the copy failed: " + _err())
            if self.M.yakamd_memcpy_d2h(out.ctypes.data, d, n * 16) != 0:
                raise RuntimeError(yak_amd._err())
        finally:
            self.M.yakamd_dev_free(d)
        return out


def gfa(table_yak, min_cnt=1, stats_only=False):
    """`yak-amd unitigs -G` through the C ABI (yak_ch_restore + yakamd_unitigs_gfa): the GFA 1 text, or with stats_only the text of
    `unitigs -s` and the G line"""
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
            out = os.path.join(d, "unitigs.gfa")
            if L.yakamd_unitigs_gfa(C.byref(o), h, out.encode()) != 0:
                raise RuntimeError("yakamd_unitigs_gfa failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
