"""Single substitution errors of reads repaired on the GPU against a count table (libyak_amd_correct.so above libyak_amd.so alone;
include/yak_amd_correct.h): the struct classes and the four device-level calls through lib(), options() for a yakamd_cropt_t,
correct() for `yak-amd correct` through the C ABI, tally() for the library's own launch tally."""
import ctypes as C
import os

import yak_amd
from yak_amd import ChT, _layer
from yak_amd._layer import P

CORRECT_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_correct.so")
CORRECT_H_SYMBOLS = [
    "yakamd_cropt_init", "yakamd_correct_find_dev", "yakamd_correct_trials_dev", "yakamd_correct_decide_dev", "yakamd_correct_image_dev", "yakamd_correct",
    "yakamd_correct_ms", "yakamd_correct_last_error", "yakamd_correct_tally_names", "yakamd_correct_tally_read", "yakamd_correct_tally_reset",
]
NOFIT, DONE, AMBIG = 0, 1, 2                   # YAKAMD_FIX_NOFIT, _DONE, _AMBIG
MS_PARTS = ("lookup", "find", "trials", "second_lookup", "decisions", "text")
TALLY_FIELDS = ("n_kmer", "n_weak", "n_cand", "n_fixed", "n_ambig", "n_nofit", "n_weak_after", "reserved")


class FixT(C.Structure):                       # yakamd_fix_t, include/yak_amd_correct.h
    _fields_ = [("at", C.c_uint64), ("seq", C.c_uint32), ("p", C.c_uint32), ("st", C.c_uint32), ("en", C.c_uint32), ("from_", C.c_uint8), ("to", C.c_uint8),
                ("fit", C.c_uint8), ("why", C.c_uint8), ("reserved", C.c_uint32)]


class CtallyT(C.Structure):                    # yakamd_ctally_t
    _fields_ = [(f, C.c_uint32) for f in TALLY_FIELDS]


class CroptT(C.Structure):                     # yakamd_cropt_t
    _fields_ = [("min_cnt", C.c_int32), ("min_run", C.c_int32), ("list", C.c_int32), ("stats_only", C.c_int32), ("chunk_size", C.c_int64)]


_lib = None


def lib():
    """Load libyak_amd_correct.so (once), after libyak_amd.so.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        V, I, L = C.c_void_p, C.c_int, C.c_int64
        _lib = _layer.load(CORRECT_LIB_PATH, yak_amd.lib, {
            **_layer.common("correct"),
            "yakamd_cropt_init": (None, [P(CroptT)]),
            "yakamd_correct_find_dev": (L, [I, I, I, V, L, V, V, L, V, L, V]),
            "yakamd_correct_trials_dev": (L, [I, V, L, V, L, V, L]),
            "yakamd_correct_decide_dev": (I, [I, I, V, V, L, V, L, V, L]),
            "yakamd_correct_image_dev": (L, [P(ChT), I, I, V, L, V, V, L, V, L, V]),
            "yakamd_correct": (I, [P(CroptT), P(ChT), C.c_char_p, C.c_char_p, C.c_char_p]), "yakamd_correct_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "correct")


def tally():
    """{kernel instantiation: launches since the last yakamd_correct_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "correct")


def ms():
    """the milliseconds of the calling thread's last yakamd_correct_image_dev or yakamd_correct: the parts of MS_PARTS in order"""
    out = (C.c_double * 6)()
    lib().yakamd_correct_ms(out)
    return list(out)


def options(min_cnt=3, min_run=1, list_fixed=False, stats_only=False, chunk_size=None):
    """a yakamd_cropt_t"""
    o = CroptT()
    lib().yakamd_cropt_init(C.byref(o))
    o.min_cnt, o.min_run, o.list, o.stats_only = min_cnt, min_run, int(bool(list_fixed)), int(bool(stats_only))
    if chunk_size is not None:
        o.chunk_size = chunk_size
    return o


def correct(table_yak, reads_fn, out_fn=None, min_cnt=3, min_run=1, list_fixed=False, stats_only=False, chunk_size=None):
    """`yak-amd correct` through the C ABI (yak_ch_restore + yakamd_correct): the corrected reads go to out_fn (None: they are returned) unless
    stats_only; returns (the reads as bytes or None, the report as bytes)"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = options(min_cnt, min_run, list_fixed, stats_only, chunk_size)
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            rep, out = os.path.join(d, "correct.txt"), out_fn or os.path.join(d, "reads.out")
            if L.yakamd_correct(C.byref(o), h, reads_fn.encode(), out.encode(), rep.encode()) != 0:
                raise RuntimeError("yakamd_correct failed: " + _err())
            reads = None
            if not stats_only and out_fn is None:
                with open(out, "rb") as f:
                    reads = f.read()
            with open(rep, "rb") as f:
                return reads, f.read()
    finally:
        M.yak_ch_destroy(h)
