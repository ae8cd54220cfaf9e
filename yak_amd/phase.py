"""The alleles of the simple bubbles phased from read support, on the GPU (libyak_amd_phase.so above libyak_amd_allele.so and the libraries below
it; include/yak_amd_phase.h): Phase(n_bubble) keeps the votes of the pairs of bubbles in device memory, takes observation
records (as yak_amd.allele.Alleles.observe() hands them out, or of the caller's own making) and the support, and hands out the pairs, the nodes,
the edges and the blocks as numpy arrays; phase() is `yak-amd bubbles -r -p` through the C ABI."""
import ctypes as C
import os

import yak_amd
import yak_amd.allele
from yak_amd import ChT, _layer
from yak_amd._layer import P
from yak_amd.allele import OBS_DTYPE, SUP_DTYPE
from yak_amd.path import _Dev

PHASE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyak_amd_phase.so")
PHASE_H_SYMBOLS = [
    "yakamd_phase_open", "yakamd_phase_stats", "yakamd_phase_votes_dev", "yakamd_phase_pairs_dev", "yakamd_phase_solve_dev", "yakamd_phase_nodes_dev",
    "yakamd_phase_edges_dev", "yakamd_phase_blocks_dev", "yakamd_phase_reset", "yakamd_phase_close", "yakamd_phase", "yakamd_phopt_init",
    "yakamd_phase_ms", "yakamd_phase_last_error", "yakamd_phase_tally_names", "yakamd_phase_tally_read", "yakamd_phase_tally_reset",
]
X, FOREST, DISC = 1, 2, 4                      # YAKAMD_PEDGE_*: the bits of an edge's flags
PAIR_DTYPE = [("i", "<u4"), ("j", "<u4"), ("cis", "<u4"), ("trans", "<u4")]
NODE_DTYPE = [("block", "<u4"), ("flags", "<u4")]
EDGE_DTYPE = [("i", "<u4"), ("j", "<u4"), ("w", "<u4"), ("flags", "<u4")]
BLOCK_DTYPE = [("block", "<u4"), ("n_bubble", "<u4"), ("n_edge", "<u4"), ("n_disc", "<u4"), ("w_sum", "<u8"), ("w_disc", "<u8")]
STATS = ("n_bubble", "n_pair", "capacity", "n_grow", "n_het", "n_edge", "n_forest", "n_block", "n_single", "n_round")


class PpairT(C.Structure):                     # yakamd_ppair_t, include/yak_amd_phase.h
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("cis", C.c_uint32), ("trans", C.c_uint32)]


class PnodeT(C.Structure):                     # yakamd_pnode_t
    _fields_ = [("block", C.c_uint32), ("flags", C.c_uint32)]


class PedgeT(C.Structure):                     # yakamd_pedge_t
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("w", C.c_uint32), ("flags", C.c_uint32)]


class PblockT(C.Structure):                    # yakamd_pblock_t
    _fields_ = [("block", C.c_uint32), ("n_bubble", C.c_uint32), ("n_edge", C.c_uint32), ("n_disc", C.c_uint32), ("w_sum", C.c_uint64), ("w_disc", C.c_uint64)]


class PhstatT(C.Structure):                    # yakamd_phstat_t
    _fields_ = [(name, C.c_uint64) for name in STATS]


class PhoptT(C.Structure):                     # yakamd_phopt_t
    _fields_ = [("min_cnt", C.c_int32), ("min_sup", C.c_int32), ("min_link", C.c_int32), ("edges", C.c_int32), ("stats_only", C.c_int32),
                ("reserved", C.c_int32), ("chunk_size", C.c_int64)]


_lib = None


def lib():
    """Load libyak_amd_phase.so (once), after the libraries below it.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        V, I = C.c_void_p, C.c_int64
        getter = (I, [V, V, I])
        _lib = _layer.load(PHASE_LIB_PATH, yak_amd.allele.lib, {
            **_layer.common("phase"),
            "yakamd_phase_open": (V, [I]), "yakamd_phase_stats": (C.c_int, [V, P(PhstatT)]),
            "yakamd_phase_votes_dev": (C.c_int, [V, V, I, P(I)]), "yakamd_phase_pairs_dev": getter,
            "yakamd_phase_solve_dev": (C.c_int, [V, V, I, C.c_int32, C.c_int32]), "yakamd_phase_nodes_dev": getter, "yakamd_phase_edges_dev": getter,
            "yakamd_phase_blocks_dev": getter, "yakamd_phase_reset": (C.c_int, [V]), "yakamd_phase_close": (None, [V]),
            "yakamd_phase": (C.c_int, [P(PhoptT), P(ChT), C.c_char_p, C.c_char_p]), "yakamd_phopt_init": (None, [P(PhoptT)]),
            "yakamd_phase_ms": (None, [P(C.c_double)])})
    return _lib


def _err():
    return _layer.last_error(lib(), "phase")


def tally():
    """{kernel instantiation: launches since the last yakamd_phase_tally_reset} of this library's own kernels"""
    return _layer.tally(lib(), "phase")


def ms():
    """the five parts of yakamd_phase_ms: compaction, votes with table growth, solve, copies, text"""
    out = (C.c_double * 5)()
    lib().yakamd_phase_ms(out)
    return [float(v) for v in out]


class Phase:
    """the votes of the pairs among n_bubble bubbles and the last solve over them: yakamd_phase_open ... yakamd_phase_close"""

    def __init__(self, n_bubble):
        self.L, self.M = lib(), yak_amd.lib()
        self.ph = self.L.yakamd_phase_open(n_bubble)
        if not self.ph:
            raise RuntimeError("yakamd_phase_open failed: " + _err())

    def close(self):
        if self.ph:
            self.L.yakamd_phase_close(self.ph)
            self.ph = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stats(self):
        st = PhstatT()
        if self.L.yakamd_phase_stats(self.ph, C.byref(st)) != 0:
            raise RuntimeError("yakamd_phase_stats failed: " + _err())
        return {name: int(getattr(st, name)) for name in STATS}

    def reset(self):
        if self.L.yakamd_phase_reset(self.ph) != 0:
            raise RuntimeError("yakamd_phase_reset failed: " + _err())

    def votes(self, obs):
        """(n_full, n_vote) of the observation records of one chunk, whose votes are added to the table"""
        import numpy as np
        obs = np.ascontiguousarray(obs, OBS_DTYPE)
        with _Dev(self.M) as dev:
            n_out = (C.c_int64 * 2)()
            if self.L.yakamd_phase_votes_dev(self.ph, dev.alloc(obs.nbytes, obs.tobytes()), len(obs), n_out) != 0:
                raise RuntimeError("yakamd_phase_votes_dev failed: " + _err())
            return int(n_out[0]), int(n_out[1])

    def solve(self, sup, min_sup=2, min_link=2):
        """the forest, the blocks and the phase from the votes so far and the support (as yak_amd.allele.Alleles.support() hands it out)"""
        import numpy as np
        sup = np.ascontiguousarray(sup, SUP_DTYPE)
        with _Dev(self.M) as dev:
            if self.L.yakamd_phase_solve_dev(self.ph, dev.alloc(sup.nbytes, sup.tobytes()), len(sup), min_sup, min_link) != 0:
                raise RuntimeError("yakamd_phase_solve_dev failed: " + _err())
        return self.stats()

    def _get(self, name, dtype, guard=0):
        """a result list through device memory of the caller's, with `guard` bytes behind it that must come back untouched"""
        import numpy as np
        get = getattr(self.L, name)
        n = get(self.ph, None, 0)
        if n < 0:
            raise RuntimeError(name + " failed: " + _err())
        out = np.zeros(n, dtype)
        if n == 0:
            return out
        with _Dev(self.M) as dev:
            fill = b"\xa5" * (out.nbytes + guard)
            d = dev.alloc(len(fill), fill)
            if get(self.ph, d, n) != n:
                raise RuntimeError(name + " failed: " + _err())
            raw = np.zeros(len(fill), np.uint8)
            dev.fetch(d, raw)
            if guard and raw[out.nbytes:].tobytes() != fill[out.nbytes:]:
                raise RuntimeError(name + " wrote behind its list")
            return np.frombuffer(raw[:out.nbytes].tobytes(), dtype).copy()

    def pairs(self, guard=0):
        """every voted pair; the order is the table's slot order and is not defined"""
        return self._get("yakamd_phase_pairs_dev", PAIR_DTYPE, guard)

    def nodes(self, guard=0):
        return self._get("yakamd_phase_nodes_dev", NODE_DTYPE, guard)

    def edges(self, guard=0):
        """the edges of the last solve; their order is not defined"""
        return self._get("yakamd_phase_edges_dev", EDGE_DTYPE, guard)

    def blocks(self, guard=0):
        return self._get("yakamd_phase_blocks_dev", BLOCK_DTYPE, guard)


def phase(table_yak, reads, min_cnt=1, min_sup=2, min_link=2, edges=False, stats_only=False, chunk_size=None):
    """`yak-amd bubbles -r -p` through the C ABI (yak_ch_restore + yakamd_phase): the header, the A, H and K lines, with edges the E lines, and
    the T line; with stats_only the header and the T line"""
    L, M = lib(), yak_amd.lib()
    h = M.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + yak_amd._err())
    try:
        o = PhoptT()
        L.yakamd_phopt_init(C.byref(o))
        o.min_cnt, o.min_sup, o.min_link, o.edges, o.stats_only = min_cnt, min_sup, min_link, int(bool(edges)), int(bool(stats_only))
        if chunk_size is not None:
            o.chunk_size = chunk_size
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "phase.txt")
            if L.yakamd_phase(C.byref(o), h, reads.encode(), out.encode()) != 0:
                raise RuntimeError("yakamd_phase failed: " + _err())
            with open(out, "rb") as f:
                return f.read()
    finally:
        M.yak_ch_destroy(h)
