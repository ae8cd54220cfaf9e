"""The compacted de Bruijn graph of a count table cleaned on the GPU: tips clipped, simple bubbles popped (libyak_amd_clean.so above
libyak_amd_bubble.so, libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so; include/yak_amd_clean.h): Clean(walk, gfa,
bubbles, k) keeps the decisions on a yak_amd.walk.Walk, its yak_amd.gfa.Gfa and its yak_amd.bubble.Bubbles in device memory and hands out the records
of the removed unitigs as a numpy array and the drop image as bytes; clean_round() is one round on a resident table; clean() is `yak-amd clean`
through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.bubble
from yak_amd import ChT, _layer
from yak_amd._layer import P

CLEAN_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_clean.so")
CLEAN_H_SYMBOLS = [
    "yakamd_cleanopt_init", "yakamd_clean_open", "yakamd_clean_stats", "yakamd_clean_records_dev", "yakamd_clean_image_dev", "yakamd_clean_close",
    "yakamd_clean_round", "yakamd_clean", "yakamd_clean_ms", "yakamd_clean_last_error", "yakamd_clean_tally_names", "yakamd_clean_tally_read",
    "yakamd_clean_tally_reset",
]
KEEP, TIP, POP = 0, 1, 2                       # YAKAMD_CLEAN_KEEP, _TIP, _POP
MS_PARTS = ("walk", "links", "bubbles", "decisions", "image", "drop_table", "subtract", "text")
ROUND_FIELDS = ("n_key", "n_unitig", "n_link", "n_bubble", "n_tip", "tip_nodes", "n_pop", "pop_nodes", "removed")
STAT_FIELDS = ("n_tip", "tip_nodes", "n_tip_kept", "n_pop", "pop_nodes", "n_pop_kept", "n_rec", "img_bytes")


class CleanRecT(C.Structure):                  # yakamd_clean_rec_t, include/yak_amd_clean.h
    _fields_ = [(f, C.c_uint64) for f in ("unitig", "why", "n_node", "kc", "other", "off")]


class CleanstatT(C.Structure):                 # yakamd_cleanstat_t
    _fields_ = [(f, C.c_uint64) for f in STAT_FIELDS]


class CleanroundT(C.Structure):                # yakamd_cleanround_t
    _fields_ = [(f, C.c_uint64) for f in ROUND_FIELDS]


class CleanoptT(C.Structure):                  # yakamd_cleanopt_t
    _fields_ = [("min_cnt", C.c_int32), ("tip_nodes", C.c_int32), ("pop_pct", C.c_int32), ("max_rounds", C.c_int32), ("list", C.c_int32)]


_lib = None


def lib():
    """Load libyak_amd_clean.so (once), after the four libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        _lib = _layer.load(CLEAN_LIB_PATH, yak_amd.bubble.lib, {
            **_layer.common("clean"),
            "yakamd_cleanopt_init": (None, [P(CleanoptT)]),
            "yakamd_clean_open": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
            "yakamd_clean_stats": (C.c_int, [C.c_void_p, P(CleanstatT)]),
            "yakamd_clean_records_dev": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
            "yakamd_clean_image_dev": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]), "yakamd_clean_close": (None, [C.c_void_p]),
            "yakamd_clean_round": (C.c_int64, [P(ChT), P(CleanoptT), P(CleanroundT)]),
            "yakamd_clean": (C.c_int, [P(CleanoptT), P(ChT), C.c_char_p, C.c_char_p]), "yakamd_clean_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "clean")


def tally():
    """{kernel instantiation: launches since the last yakamd_clean_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "clean")


def ms():
    """the milliseconds of the calling thread's last open, round or command, summed over its rounds: the parts of MS_PARTS in order"""
    out = (C.c_double * 8)()
    lib().yakamd_clean_ms(out)
    return list(out)


def options(min_cnt=1, tip_nodes=None, pop_pct=100, max_rounds=8, list_removed=False):
    """a yakamd_cleanopt_t; tip_nodes None: the table's k"""
    o = CleanoptT()
    lib().yakamd_cleanopt_init(C.byref(o))
    o.min_cnt, o.pop_pct, o.max_rounds, o.list = min_cnt, pop_pct, max_rounds, int(bool(list_removed))
    if tip_nodes is not None:
        o.tip_nodes = tip_nodes
    return o


class Clean:
    """the decisions of one round on a device walk (a yak_amd.walk.Walk), its links (a yak_amd.gfa.Gfa) and its bubbles (a yak_amd.bubble.Bubbles)
    at the table's k: yakamd_clean_open ... yakamd_clean_close.  Copies are taken at the open: the records and the image outlive all three"""

    def __init__(self, walk, gfa, bubbles, k, tip_nodes=None, pop_pct=100):
        self.L, self.M = lib(), yak_amd.lib()
        self.c = self.L.yakamd_clean_open(walk.w if walk is not None else None, gfa.g if gfa is not None else None, bubbles.b if bubbles is not None else None, k,
                                          k if tip_nodes is None else tip_nodes, pop_pct)
        if not self.c:
            raise RuntimeError("yakamd_clean_open failed: " + _err())

    def close(self):
        if self.c:
            self.L.yakamd_clean_close(self.c)
            self.c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = CleanstatT()
        if self.L.yakamd_clean_stats(self.c, C.byref(st)) != 0:
            raise RuntimeError("yakamd_clean_stats failed: " + _err())
        return {f: int(getattr(st, f)) for f in STAT_FIELDS}

    def _fetch(self, get, n_bytes_of, out_of):
        n = get(self.c, None, 0)
        if n < 0:
            raise RuntimeError("the size query failed: " + _err())
        out = out_of(n)
        if n == 0:
            return out
        d = self.M.yakamd_dev_alloc(n_bytes_of(n))
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + yak_amd._err())
        try:
            if get(self.c, d, n) != n:
                raise RuntimeError("the copy failed: " + _err())
            if self.M.yakamd_memcpy_d2h(out.ctypes.data, d, n_bytes_of(n)) != 0:
                raise RuntimeError(yak_amd._err())
        finally:
            self.M.yakamd_dev_free(d)
        return out

    def records(self):
        """the removed unitigs ascending by unitig: why (TIP or POP), n_node, kc, other (the anchor end of a tip, the winning arm's end of a popped
        arm: unitig << 1 | (1 for '-')), off (where its bases start in the image).  Through device memory of the caller's"""
        import numpy as np
        dtype = np.dtype([(f, "<u8") for f in ("unitig", "why", "n_node", "kc", "other", "off")])
        return self._fetch(self.L.yakamd_clean_records_dev, lambda n: n * 48, lambda n: np.zeros(n, dtype))

    def image(self):
        """the drop image: the removed unitigs' bases in record order, each followed by a newline"""
        import numpy as np
        return self._fetch(self.L.yakamd_clean_image_dev, lambda n: n, lambda n: np.zeros(n, np.uint8)).tobytes()


def clean_round(table, min_cnt=1, tip_nodes=None, pop_pct=100):
    """one round on a resident yak_amd.Table (yakamd_clean_round): the round's tallies as a dict; the table has lost `removed` k-mers"""
    o = options(min_cnt, tip_nodes, pop_pct)
    st = CleanroundT()
    n = lib().yakamd_clean_round(table.h, C.byref(o), C.byref(st))
    if n < 0:
        raise RuntimeError("yakamd_clean_round failed: " + _err())
    return {f: int(getattr(st, f)) for f in ROUND_FIELDS}


def clean(table_yak, out_yak, min_cnt=1, tip_nodes=None, pop_pct=100, max_rounds=8, list_removed=False):
    """`yak-amd clean` through the C ABI (yak_ch_restore + yakamd_clean): writes the cleaned table to out_yak and returns the report"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = options(min_cnt, tip_nodes, pop_pct, max_rounds, list_removed)
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            rep = os.path.join(d, "clean.txt")
            if L.yakamd_clean(C.byref(o), h, out_yak.encode(), rep.encode()) != 0:
                raise RuntimeError("yakamd_clean failed: " + _err())
            with open(rep, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
