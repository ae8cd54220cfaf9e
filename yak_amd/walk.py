"""The unitigs of a count table's de Bruijn graph walked on the GPU (libyak_amd_walk.so beside libyak_amd.so; include/yak_amd_walk.h; DESIGN.md
section 21): Walk(table, min_cnt) keeps the node -> unitig map, the descriptors and the bases in device memory and hands them out as numpy arrays;
unitigs_dev() is `yak-amd unitigs -g` through the C ABI."""
import ctypes as C
import os

import yak_amd
from yak_amd import ChT, GstatT, UgoptT, _layer
from yak_amd._layer import P

WALK_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_walk.so")
WALK_H_SYMBOLS = [
    "yakamd_uwalk_open", "yakamd_uwalk_stats", "yakamd_uwalk_gstat", "yakamd_uwalk_map_dev", "yakamd_uwalk_desc_dev", "yakamd_uwalk_bases_dev",
    "yakamd_uwalk_close", "yakamd_unitigs_dev", "yakamd_uwalk_ms", "yakamd_walk_last_error", "yakamd_walk_tally_names", "yakamd_walk_tally_read",
    "yakamd_walk_tally_reset",
]
STAT_FIELDS = ("n_key", "n_node", "n_open", "n_cycle", "sum_len", "max_len", "n50", "rounds", "host_nodes")


class UwstatT(C.Structure):                    # yakamd_uwstat_t, include/yak_amd_walk.h
    _fields_ = [(f, C.c_uint64) for f in STAT_FIELDS]


_lib = None


def lib():
    """Load libyak_amd_walk.so (once), after libyak_amd.so.  Raises if it has not been built: there is no fallback to the host walk."""
    global _lib
    if _lib is None:
        dev = (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64])
        _lib = _layer.load(WALK_LIB_PATH, yak_amd.lib, {
            **_layer.common("walk"),
            "yakamd_uwalk_open": (C.c_void_p, [P(ChT), C.c_int]), "yakamd_uwalk_stats": (C.c_int, [C.c_void_p, P(UwstatT)]),
            "yakamd_uwalk_gstat": (C.c_int, [C.c_void_p, P(GstatT)]), "yakamd_uwalk_map_dev": dev, "yakamd_uwalk_desc_dev": dev,
            "yakamd_uwalk_bases_dev": dev, "yakamd_uwalk_close": (None, [C.c_void_p]), "yakamd_unitigs_dev": (C.c_int, [P(UgoptT), P(ChT), C.c_char_p]),
            "yakamd_uwalk_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "walk")


def tally():
    """{kernel instantiation: launches since the last yakamd_walk_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "walk")


class Walk:
    """the device walk of a table (a yak_amd.Table): yakamd_uwalk_open ... yakamd_uwalk_close"""

    def __init__(self, table, min_cnt=1):
        self.L, self.M = lib(), yak_amd.lib()
        self.w = self.L.yakamd_uwalk_open(table.h, min_cnt)
        if not self.w:
            raise RuntimeError("yakamd_uwalk_open failed: " + _err())

    def close(self):
        if self.w:
            self.L.yakamd_uwalk_close(self.w)
            self.w = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = UwstatT()
        if self.L.yakamd_uwalk_stats(self.w, C.byref(st)) != 0:
            raise RuntimeError("yakamd_uwalk_stats failed: " + _err())
        return {f: int(getattr(st, f)) for f in STAT_FIELDS}

    def gstat(self):
        st = GstatT()
        if self.L.yakamd_uwalk_gstat(self.w, C.byref(st)) != 0:
            raise RuntimeError("yakamd_uwalk_gstat failed: " + _err())
        return dict(n_key=st.n_key, n_node=st.n_node, n_arc=st.n_arc, n_linked_side=st.n_linked_side, deg=[[st.deg[l][r] for r in range(5)] for l in range(5)])

    def _array(self, getter, dtype):
        """a result through device memory of the caller's, the way Table.graph_nodes gets its records"""
        import numpy as np
        dtype = np.dtype(dtype)
        n = getter(self.w, None, 0)
        if n < 0:
            raise RuntimeError("the size query failed: " + _err())
        out = np.zeros(n, dtype)
        if n == 0:
            return out
        d = self.M.yakamd_dev_alloc(n * dtype.itemsize)
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + yak_amd._err())
        try:
            if getter(self.w, d, n) != n:
                raise RuntimeError("the copy failed: " + _err())
            if self.M.yakamd_memcpy_d2h(out.ctypes.data, d, n * dtype.itemsize) != 0:
                raise RuntimeError(yak_amd._err())
        finally:
            self.M.yakamd_dev_free(d)
        return out

    def map(self):
        """per stored key in listing order: (unitig, at = p << 1 | d); (2^64 - 1, 0) for a key that is no node"""
        return self._array(self.L.yakamd_uwalk_map_dev, [("unitig", "<u8"), ("at", "<u8")])

    def desc(self):
        """per unitig: (off, n_node, kc, first = v_0 << 1 | cycle)"""
        return self._array(self.L.yakamd_uwalk_desc_dev, [("off", "<u8"), ("n_node", "<u8"), ("kc", "<u8"), ("first", "<u8")])

    def bases(self):
        """ASCII ACGT, the unitigs back to back (uint8)"""
        return self._array(self.L.yakamd_uwalk_bases_dev, "u1")


def unitigs_dev(table_yak, min_cnt=1, stats_only=False):
    """`yak-amd unitigs -g` through the C ABI (yak_ch_restore + yakamd_unitigs_dev): byte for byte the text of yak_amd.unitigs()"""
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
            out = os.path.join(d, "unitigs.txt")
            if L.yakamd_unitigs_dev(C.byref(o), h, out.encode()) != 0:
                raise RuntimeError("yakamd_unitigs_dev failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
