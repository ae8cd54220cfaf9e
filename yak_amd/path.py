"""Sequences laid onto the unitig graph of a count table as paths, on the GPU (libyak_amd_path.so beside libyak_amd_walk.so and libyak_amd.so;
include/yak_amd_path.h): Path(walk, k) keeps an index of every node of a yak_amd.walk.Walk in device memory and turns base
images into hit arrays and those into paths, handed out as numpy arrays; paths() is `yak-amd paths` through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.walk
from yak_amd import ChT, _layer
from yak_amd._layer import P

PATH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_path.so")
PATH_H_SYMBOLS = [
    "yakamd_path_open", "yakamd_path_stats", "yakamd_path_hits_dev", "yakamd_path_chain_dev", "yakamd_path_close", "yakamd_paths", "yakamd_ppopt_init",
    "yakamd_path_ms", "yakamd_path_last_error", "yakamd_path_tally_names", "yakamd_path_tally_read", "yakamd_path_tally_reset",
]
NONE, ABSENT = (1 << 64) - 1, (1 << 64) - 2
TILE = 1024                                    # PX_TILE of yak_amd/path/path_step.h: the positions a workgroup serves
PATH_DTYPE = [("step_off", "<u8"), ("ps", "<u8"), ("seq", "<u4"), ("n_step", "<u4"), ("qs", "<u4"), ("qe", "<u4")]
TALLY_DTYPE = [("n_kmer", "<u4"), ("n_hit", "<u4"), ("n_path", "<u4"), ("n_step", "<u4")]


class PxstatT(C.Structure):                    # yakamd_pxstat_t, include/yak_amd_path.h
    _fields_ = [("n_unitig", C.c_uint64), ("n_node", C.c_uint64), ("table_slots", C.c_uint64), ("max_probe", C.c_uint64)]


class PpoptT(C.Structure):                     # yakamd_ppopt_t
    _fields_ = [("min_cnt", C.c_int32), ("min_len", C.c_int32), ("stats_only", C.c_int32), ("reserved", C.c_int32), ("chunk_size", C.c_int64)]


_lib = None


def lib():
    """Load libyak_amd_path.so (once), after the two libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        V = C.c_void_p
        _lib = _layer.load(PATH_LIB_PATH, yak_amd.walk.lib, {
            **_layer.common("path"),
            "yakamd_path_open": (V, [V, C.c_int]), "yakamd_path_stats": (C.c_int, [V, P(PxstatT)]),
            "yakamd_path_hits_dev": (C.c_int, [V, V, C.c_int64, V]),
            "yakamd_path_chain_dev": (C.c_int, [V, V, C.c_int64, V, V, C.c_int64, V, C.c_int64, V, C.c_int64, V, P(C.c_int64)]),
            "yakamd_path_close": (None, [V]), "yakamd_paths": (C.c_int, [P(PpoptT), P(ChT), C.c_char_p, C.c_char_p]),
            "yakamd_ppopt_init": (None, [P(PpoptT)]), "yakamd_path_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "path")


def tally():
    """{kernel instantiation: launches since the last yakamd_path_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "path")


def ms():
    """the six parts of yakamd_path_ms: index, hits, count and scan, emit, copies, text"""
    out = (C.c_double * 6)()
    lib().yakamd_path_ms(out)
    return [float(v) for v in out]


class _Dev:
    """device memory of the caller's for the length of a call"""

    def __init__(self, M):
        self.M, self.held = M, []

    def alloc(self, nbytes, src=None):
        d = self.M.yakamd_dev_alloc(max(int(nbytes), 16))
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + yak_amd._err())
        self.held.append(d)
        if src is not None and len(src) and self.M.yakamd_memcpy_h2d(d, src, len(src)) != 0:
            raise RuntimeError(yak_amd._err())
        return d

    def fetch(self, d, arr):
        if arr.nbytes and self.M.yakamd_memcpy_d2h(arr.ctypes.data, d, arr.nbytes) != 0:
            raise RuntimeError(yak_amd._err())
        return arr

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for d in self.held:
            self.M.yakamd_dev_free(d)


class Path:
    """the index of a device walk (a yak_amd.walk.Walk) at its table's k: yakamd_path_open ... yakamd_path_close"""

    def __init__(self, walk, k):
        self.L, self.M = lib(), yak_amd.lib()
        self.px = self.L.yakamd_path_open(walk.w if walk is not None else None, k)
        if not self.px:
            raise RuntimeError("yakamd_path_open failed: " + _err())

    def close(self):
        if self.px:
            self.L.yakamd_path_close(self.px)
            self.px = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = PxstatT()
        if self.L.yakamd_path_stats(self.px, C.byref(st)) != 0:
            raise RuntimeError("yakamd_path_stats failed: " + _err())
        return dict(n_unitig=int(st.n_unitig), n_node=int(st.n_node), table_slots=int(st.table_slots), max_probe=int(st.max_probe))

    def _hits_dev(self, dev, image):
        n = len(image)
        n16 = (n + 15) & ~15
        d_img = dev.alloc(n16, bytes(image) + b"\n" * (n16 - n))
        d_hit = dev.alloc(n16 * 8)
        if self.L.yakamd_path_hits_dev(self.px, d_img, n, d_hit) != 0:
            raise RuntimeError("yakamd_path_hits_dev failed: " + _err())
        return d_hit, n16

    def hits(self, image):
        """hit[i] of every byte of a base image (bytes; each sequence followed by a newline): NONE, ABSENT or unitig << 32 | p << 1 | o"""
        import numpy as np
        with _Dev(self.M) as dev:
            d_hit, n16 = self._hits_dev(dev, image)
            return dev.fetch(d_hit, np.zeros(n16, np.uint64))[:len(image)]

    def chain(self, image, off, length):
        """(paths, steps, tally) of a base image whose sequence s is image[off[s] : off[s] + length[s]]: the path records and the steps in image
        order, one tally per sequence"""
        import numpy as np
        off, length = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(length, np.uint32)
        n, n_seq = len(image), len(off)
        with _Dev(self.M) as dev:
            d_hit, _ = self._hits_dev(dev, image)
            d_off, d_len, d_tally = dev.alloc(n_seq * 8, off.tobytes()), dev.alloc(n_seq * 4, length.tobytes()), dev.alloc(n_seq * 16)
            n_out = (C.c_int64 * 2)()
            rc = self.L.yakamd_path_chain_dev(self.px, d_hit, n, d_off, d_len, n_seq, None, 0, None, 0, d_tally, n_out)
            if rc < 0:
                raise RuntimeError("yakamd_path_chain_dev failed: " + _err())
            paths, steps, tally = np.zeros(n_out[0], PATH_DTYPE), np.zeros(n_out[1], np.uint64), np.zeros(n_seq, TALLY_DTYPE)
            dev.fetch(d_tally, tally)
            if n_out[0]:
                d_paths, d_steps = dev.alloc(paths.nbytes), dev.alloc(steps.nbytes)
                again = (C.c_int64 * 2)()
                if self.L.yakamd_path_chain_dev(self.px, d_hit, n, d_off, d_len, n_seq, d_paths, n_out[0], d_steps, n_out[1], None, again) != 0:
                    raise RuntimeError("yakamd_path_chain_dev failed: " + _err())
                dev.fetch(d_paths, paths)
                dev.fetch(d_steps, steps)
            return paths, steps, tally


def paths(table_yak, fn, min_cnt=1, min_len=0, stats_only=False, chunk_size=None):
    """`yak-amd paths` through the C ABI (yak_ch_restore + yakamd_paths): the GAF text, or with stats_only the tallies per sequence"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = PpoptT()
        L.yakamd_ppopt_init(C.byref(o))
        o.min_cnt, o.min_len, o.stats_only = min_cnt, min_len, int(bool(stats_only))
        if chunk_size is not None:
            o.chunk_size = chunk_size
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "paths.gaf")
            if L.yakamd_paths(C.byref(o), h, fn.encode(), out.encode()) != 0:
                raise RuntimeError("yakamd_paths failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
