"""The alleles of the simple bubbles supported with reads, on the GPU (libyak_amd_allele.so above libyak_amd_path.so, libyak_amd_bubble.so and the
three libraries below them; include/yak_amd_allele.h): Alleles(walk, bubbles) keeps the arm map of a yak_amd.walk.Walk and
its yak_amd.bubble.Bubbles and the support of every bubble in device memory, turns path records and steps into observation records, handed out as
numpy arrays, and adds them to the support; alleles() is `yak-amd bubbles -r` through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.bubble
import yak_amd.path
from yak_amd import ChT, _layer
from yak_amd._layer import P
from yak_amd.path import PATH_DTYPE, _Dev

ALLELE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_allele.so")
ALLELE_H_SYMBOLS = [
    "yakamd_allele_open", "yakamd_allele_stats", "yakamd_allele_obs_dev", "yakamd_allele_support_dev", "yakamd_allele_reset", "yakamd_allele_close",
    "yakamd_alleles", "yakamd_alopt_init", "yakamd_allele_ms", "yakamd_allele_last_error", "yakamd_allele_tally_names", "yakamd_allele_tally_read",
    "yakamd_allele_tally_reset",
]
A, FULL, REV = 1, 2, 4                         # YAKAMD_AOBS_*: the bits of flags
OBS_DTYPE = [("seq", "<u4"), ("bubble", "<u4"), ("flags", "<u4"), ("path", "<u4")]
SUP_DTYPE = [("full", "<u8", 2), ("part", "<u8", 2)]


class AobsT(C.Structure):                      # yakamd_aobs_t, include/yak_amd_allele.h
    _fields_ = [("seq", C.c_uint32), ("bubble", C.c_uint32), ("flags", C.c_uint32), ("path", C.c_uint32)]


class AsupT(C.Structure):                      # yakamd_asup_t
    _fields_ = [("full", C.c_uint64 * 2), ("part", C.c_uint64 * 2)]


class AlstatT(C.Structure):                    # yakamd_alstat_t
    _fields_ = [("n_unitig", C.c_uint64), ("n_bubble", C.c_uint64), ("n_arm", C.c_uint64)]


class AloptT(C.Structure):                     # yakamd_alopt_t
    _fields_ = [("min_cnt", C.c_int32), ("min_sup", C.c_int32), ("min_frag", C.c_int32), ("fragments", C.c_int32), ("stats_only", C.c_int32),
                ("reserved", C.c_int32), ("chunk_size", C.c_int64)]


_lib = None


def _below():
    yak_amd.path.lib()
    yak_amd.bubble.lib()


def lib():
    """Load libyak_amd_allele.so (once), after the five libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        V = C.c_void_p
        _lib = _layer.load(ALLELE_LIB_PATH, _below, {
            **_layer.common("allele"),
            "yakamd_allele_open": (V, [V, V]), "yakamd_allele_stats": (C.c_int, [V, P(AlstatT)]),
            "yakamd_allele_obs_dev": (C.c_int, [V, V, C.c_int64, V, C.c_int64, V, C.c_int64, P(C.c_int64)]),
            "yakamd_allele_support_dev": (C.c_int64, [V, V, C.c_int64]), "yakamd_allele_reset": (C.c_int, [V]), "yakamd_allele_close": (None, [V]),
            "yakamd_alleles": (C.c_int, [P(AloptT), P(ChT), C.c_char_p, C.c_char_p]), "yakamd_alopt_init": (None, [P(AloptT)]),
            "yakamd_allele_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "allele")


def tally():
    """{kernel instantiation: launches since the last yakamd_allele_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "allele")


def ms():
    """the five parts of yakamd_allele_ms: arm map, count and scan, emit, copies, text"""
    out = (C.c_double * 5)()
    lib().yakamd_allele_ms(out)
    return [float(v) for v in out]


class Alleles:
    """the arm map of a device walk (a yak_amd.walk.Walk) and its bubbles (a yak_amd.bubble.Bubbles), and the support of every bubble:
    yakamd_allele_open ... yakamd_allele_close.  A copy of the records is taken at the open: the map outlives the walk and the bubbles"""

    def __init__(self, walk, bubbles):
        self.L, self.M = lib(), yak_amd.lib()
        self.al = self.L.yakamd_allele_open(walk.w if walk is not None else None, bubbles.b if bubbles is not None else None)
        if not self.al:
            raise RuntimeError("yakamd_allele_open failed: " + _err())

    def close(self):
        if self.al:
            self.L.yakamd_allele_close(self.al)
            self.al = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = AlstatT()
        if self.L.yakamd_allele_stats(self.al, C.byref(st)) != 0:
            raise RuntimeError("yakamd_allele_stats failed: " + _err())
        return dict(n_unitig=int(st.n_unitig), n_bubble=int(st.n_bubble), n_arm=int(st.n_arm))

    def reset(self):
        if self.L.yakamd_allele_reset(self.al) != 0:
            raise RuntimeError("yakamd_allele_reset failed: " + _err())

    def observe(self, paths, steps, count_only=False):
        """(records, n_obs, n_full) of the paths and steps of a chunk (as yak_amd.path.Path.chain() hands them out); the records are added to
        the support unless count_only, which returns no record"""
        import numpy as np
        paths, steps = np.ascontiguousarray(paths, PATH_DTYPE), np.ascontiguousarray(steps, np.uint64)
        with _Dev(self.M) as dev:
            d_paths, d_steps = dev.alloc(paths.nbytes, paths.tobytes()), dev.alloc(steps.nbytes, steps.tobytes())
            n_out = (C.c_int64 * 2)()
            rc = self.L.yakamd_allele_obs_dev(self.al, d_paths, len(paths), d_steps, len(steps), None, 0, n_out)
            if rc < 0:
                raise RuntimeError("yakamd_allele_obs_dev failed: " + _err())
            obs = np.zeros(0 if count_only else n_out[0], OBS_DTYPE)
            if not count_only and n_out[0]:
                d_obs = dev.alloc(obs.nbytes)
                again = (C.c_int64 * 2)()
                if self.L.yakamd_allele_obs_dev(self.al, d_paths, len(paths), d_steps, len(steps), d_obs, n_out[0], again) != 0 or list(again) != list(n_out):
                    raise RuntimeError("yakamd_allele_obs_dev failed: " + _err())
                dev.fetch(d_obs, obs)
            return obs, int(n_out[0]), int(n_out[1])

    def support(self):
        """full[2] and part[2] of every bubble, in list order.  Through device memory of the caller's, as Bubbles.records() gets its entries"""
        import numpy as np
        n = self.L.yakamd_allele_support_dev(self.al, None, 0)
        if n < 0:
            raise RuntimeError("the size query failed: " + _err())
        out = np.zeros(n, SUP_DTYPE)
        if n == 0:
            return out
        with _Dev(self.M) as dev:
            d = dev.alloc(n * 32)
            if self.L.yakamd_allele_support_dev(self.al, d, n) != n:
                raise RuntimeError("the copy failed: " + _err())
            return dev.fetch(d, out)


def alleles(table_yak, reads, min_cnt=1, min_sup=2, min_frag=1, fragments=False, stats_only=False, chunk_size=None):
    """`yak-amd bubbles -r` through the C ABI (yak_ch_restore + yakamd_alleles): the header, the F lines with fragments, the A lines and the T
    line; with stats_only the header and the T line"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = AloptT()
        L.yakamd_alopt_init(C.byref(o))
        o.min_cnt, o.min_sup, o.min_frag, o.fragments, o.stats_only = min_cnt, min_sup, min_frag, int(bool(fragments)), int(bool(stats_only))
        if chunk_size is not None:
            o.chunk_size = chunk_size
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "alleles.txt")
            if L.yakamd_alleles(C.byref(o), h, reads.encode(), out.encode()) != 0:
                raise RuntimeError("yakamd_alleles failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
