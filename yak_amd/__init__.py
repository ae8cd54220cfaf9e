"""yak_amd -- MI355X-native k-mer counting engine behind lh3/yak's C API.

This package is only the Python-side loader used by tests and bench.py.  The product is the
C-ABI shared library ``yak_amd/libyak_amd.so`` (hand-written gfx950 HIP kernels + the drop-in
``yak.h`` surface declared in ``include/yak.h`` / ``include/yak_amd.h``).  There is no Python or
CPU implementation of the counting path here: if the library is missing, importing :func:`lib`
raises; if no MI355X is visible, ``yak_ch_init`` / ``yak_count`` return NULL and the wrappers raise.

Note for processes that also use PyTorch-ROCm: import torch BEFORE calling :func:`lib` (torch ships
its own copy of the HIP runtime; whichever is loaded first serves both).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libyak_amd.so")

# every symbol include/yak.h and include/yak_amd.h declare (checked by tests/test_abi.py)
YAK_H_SYMBOLS = [
    "yak_copt_init", "yak_bf_init", "yak_bf_destroy", "yak_bf_insert",
    "yak_ch_init", "yak_ch_destroy", "yak_ch_destroy_bf", "yak_ch_insert_list", "yak_ch_get",
    "yak_ch_inc", "yak_ch_getseq", "yak_ch_clear", "yak_ch_hist", "yak_ch_shrink", "yak_ch_dump",
    "yak_ch_restore", "yak_count", "yak_verbose", "seq_nt4_table", "yak_qopt_init", "yak_qv", "yak_recount", "yak_ch_setcnt",
    "yak_ch_tighten", "yak_ch_merge", "yak_ch_subtract", "yak_ch_isec", "yak_ch_restore_core", "yak_qv_solve",
]
YAK_AMD_H_SYMBOLS = [
    "yakamd_device_count", "yakamd_last_error", "yakamd_ctx_of", "yakamd_set_shard",
    "yakamd_pass_begin", "yakamd_feed_bases_dev", "yakamd_feed_bases_host", "yakamd_feed_packed_dev", "yakamd_pack_bases_dev", "yakamd_packed_bytes", "yakamd_pack_bases_host", "yakamd_feed_packed_host", "yakamd_feed_packed_pieces_host", "yakamd_feed_hashed_dev",
    "yakamd_pass_end", "yakamd_extract_dev", "yakamd_sync_host", "yakamd_dump_mem", "yakamd_dump_range_mem", "yakamd_subtable",
    "yakamd_get_stats", "yakamd_trim", "yakamd_peak_bytes", "yakamd_dev_alloc", "yakamd_dev_free", "yakamd_memcpy_h2d",
    "yakamd_memcpy_d2h", "yakamd_partition_dev", "yakamd_feed_partitioned_dev", "yakamd_debug_counters", "yakamd_count_hashes_dev",
    "yakamd_partition_hashes_dev", "yakamd_count_partitioned_dev", "yakamd_feed_partitioned_lent_dev",
    "yakamd_tagged_ok", "yakamd_pass_fast", "yakamd_partition_tagged_dev", "yakamd_feed_partitioned_tagged_dev",
    "yakamd_lookup_dev", "yakamd_qv_reduce_dev", "yakamd_host_image", "yakamd_host_image_packed", "yakamd_gz_tune", "yakamd_gz_inflate", "yakamd_test_set", "yakamd_test_reset", "yakamd_tally_names", "yakamd_tally_read", "yakamd_tally_reset",
    "yakamd_retain_input", "yakamd_count_retained", "yakamd_retained_instances", "yakamd_count_multi_dev",
    "yakamd_host_alloc", "yakamd_host_free", "yakamd_device_sync", "yakamd_mem_info", "yakamd_last_sweeps", "yakamd_pool_report",
    "yakamd_triobin_lookup_dev", "yakamd_triobin_reduce_dev", "yakamd_tbopt_init", "yakamd_triobin",
    "yakamd_trioeval_reduce_dev", "yakamd_teopt_init", "yakamd_trioeval",
    "yakamd_inspect_dev", "yakamd_inopt_init", "yakamd_inspect", "yakamd_inspect_tables",
    "yakamd_chkerr_lookup_dev", "yakamd_chkerr_streaks_dev", "yakamd_ceopt_init", "yakamd_chkerr",
    "yakamd_sexchr_reduce_dev", "yakamd_scopt_init", "yakamd_sexchr",
    "yakamd_kmers_dev", "yakamd_print_dev", "yakamd_propt_init", "yakamd_print", "yakamd_host_syncs",
    "yakamd_ch_sum", "yakamd_yak_header",
    "yakamd_depth_reduce_dev", "yakamd_dpopt_init", "yakamd_depth",
    "yakamd_cover_dev", "yakamd_cvopt_init", "yakamd_cover",
    "yakamd_hetmers_dev", "yakamd_hetmer_pairs_dev", "yakamd_hmopt_init", "yakamd_hetmers",
    "yakamd_graph_open", "yakamd_graph_stats", "yakamd_graph_nodes_dev", "yakamd_graph_close", "yakamd_graph_open_ms", "yakamd_ugopt_init", "yakamd_unitigs", "yakamd_unitigs_ms",
    "yakamd_hpc_dev", "yakamd_hpc_packed_dev", "yakamd_hpc_host", "yakamd_ch_set_hpc", "yakamd_ch_hpc", "yakamd_count_hpc",
]


class CoptT(C.Structure):                      # yak_copt_t, include/yak.h (reference yak.h:25-31)
    _fields_ = [("bf_shift", C.c_int32), ("bf_n_hash", C.c_int32), ("k", C.c_int32),
                ("pre", C.c_int32), ("n_thread", C.c_int32), ("chunk_size", C.c_int64)]


class ChT(C.Structure):                        # yak_ch_t (reference yak.h:61-65)
    _fields_ = [("k", C.c_int), ("pre", C.c_int), ("n_hash", C.c_int), ("n_shift", C.c_int),
                ("tot", C.c_uint64), ("h", C.c_void_p)]


class QoptT(C.Structure):                      # yak_qopt_t (reference yak.h:33-40)
    _fields_ = [("print_each", C.c_int32), ("print_err_kmer", C.c_int32), ("min_len", C.c_int32),
                ("n_threads", C.c_int32), ("min_frac", C.c_double), ("fpr", C.c_double), ("chunk_size", C.c_int64)]


class QstatT(C.Structure):                     # yak_qstat_t (reference yak.h:42-47)
    _fields_ = [("tot", C.c_int64), ("qv_raw", C.c_double), ("qv", C.c_double), ("cov", C.c_double), ("err", C.c_double),
                ("fpr_lower", C.c_double), ("fpr_upper", C.c_double), ("adj_cnt", C.c_double * 1024)]


class TboptT(C.Structure):                     # yakamd_tbopt_t, include/yak_amd.h
    _fields_ = [("ratio_thres", C.c_double), ("print_diff", C.c_int32), ("n_threads", C.c_int32), ("chunk_size", C.c_int64)]


class TeoptT(C.Structure):                     # yakamd_teopt_t, include/yak_amd.h
    _fields_ = [("min_n", C.c_int32), ("print_err", C.c_int32), ("print_frag", C.c_int32), ("n_threads", C.c_int32),
                ("chunk_size", C.c_int64)]


class InoptT(C.Structure):                     # yakamd_inopt_t, include/yak_amd.h
    _fields_ = [("max_cnt", C.c_int32), ("ref_probe", C.c_int32), ("n_threads", C.c_int32), ("batch_keys", C.c_int64)]


class CeoptT(C.Structure):                     # yakamd_ceopt_t, include/yak_amd.h
    _fields_ = [("min_cnt", C.c_int32), ("min_streak", C.c_int32), ("n_threads", C.c_int32), ("chunk_size", C.c_int64)]


class ScoptT(C.Structure):                     # yakamd_scopt_t, include/yak_amd.h
    _fields_ = [("n_threads", C.c_int32), ("chunk_size", C.c_int64)]


class PropT(C.Structure):                      # yakamd_propt_t, include/yak_amd.h
    _fields_ = [("with_counts", C.c_int32), ("n_threads", C.c_int32), ("batch_bytes", C.c_int64)]


class DpoptT(C.Structure):                     # yakamd_dpopt_t, include/yak_amd.h
    _fields_ = [("window", C.c_int64), ("n_threads", C.c_int32), ("chunk_size", C.c_int64)]


class WinT(C.Structure):                       # yakamd_win_t, include/yak_amd.h
    _fields_ = [("n_kmer", C.c_uint32), ("n_present", C.c_uint32), ("median", C.c_uint32), ("max", C.c_uint32), ("sum", C.c_uint64)]


class HmoptT(C.Structure):                     # yakamd_hmopt_t, include/yak_amd.h
    _fields_ = [("min_cnt", C.c_int32), ("print_pairs", C.c_int32), ("batch_keys", C.c_int64)]


class HetpairT(C.Structure):                   # yakamd_hetpair_t, include/yak_amd.h
    _fields_ = [("x", C.c_uint64), ("y", C.c_uint64), ("cx", C.c_uint32), ("cy", C.c_uint32)]


class GstatT(C.Structure):                     # yakamd_gstat_t, include/yak_amd.h
    _fields_ = [("n_key", C.c_uint64), ("n_node", C.c_uint64), ("n_arc", C.c_uint64), ("n_linked_side", C.c_uint64), ("deg", (C.c_uint64 * 5) * 5)]


class GnodeT(C.Structure):                     # yakamd_gnode_t, include/yak_amd.h
    _fields_ = [("x", C.c_uint64), ("link", C.c_uint64 * 2), ("count", C.c_uint32), ("edges", C.c_uint32)]


class UgoptT(C.Structure):                     # yakamd_ugopt_t, include/yak_amd.h
    _fields_ = [("min_cnt", C.c_int32), ("stats_only", C.c_int32), ("n_threads", C.c_int32), ("batch_keys", C.c_int64)]


class CvoptT(C.Structure):                     # yakamd_cvopt_t, include/yak_amd.h
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("intervals", C.c_int32), ("mask", C.c_int32), ("invert", C.c_int32), ("min_hit", C.c_int64),
                ("min_frac", C.c_double), ("n_threads", C.c_int32), ("chunk_size", C.c_int64)]


class CovT(C.Structure):                       # yakamd_cov_t, include/yak_amd.h
    _fields_ = [("n_kmer", C.c_uint32), ("n_hit", C.c_uint32), ("n_cov", C.c_uint32), ("n_run", C.c_uint32)]


class StreakT(C.Structure):                    # yakamd_streak_t, include/yak_amd.h
    _fields_ = [("seq", C.c_uint32), ("st", C.c_uint32), ("en", C.c_uint32), ("type", C.c_uint32)]


class StatsT(C.Structure):                     # yakamd_stats_t
    _fields_ = [("ms_extract", C.c_double), ("ms_insert", C.c_double), ("ms_bloom", C.c_double),
                ("ms_select", C.c_double), ("ms_sort", C.c_double), ("ms_replay", C.c_double),
                ("ms_total", C.c_double), ("ms_dominant_kernel", C.c_double),
                ("n_dominant_launches", C.c_int64), ("n_instances", C.c_int64),
                ("n_distinct_seen", C.c_int64), ("n_new_keys", C.c_int64),
                ("n_bloom_candidates", C.c_int64), ("ms_part2", C.c_double), ("ms_shrink", C.c_double),
                ("pass2_path", C.c_int64)]


_lib = None


def lib():
    """Load libyak_amd.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make lib` "
                           "(python __graft_entry__.py build); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.yak_copt_init.argtypes = [P(CoptT)]
    L.yak_ch_init.restype = P(ChT); L.yak_ch_init.argtypes = [C.c_int] * 4
    L.yak_ch_destroy.argtypes = [P(ChT)]
    L.yak_ch_destroy_bf.argtypes = [P(ChT)]
    L.yak_ch_insert_list.restype = C.c_int
    L.yak_ch_insert_list.argtypes = [P(ChT), C.c_int, C.c_int, P(C.c_uint64)]
    L.yak_ch_get.restype = C.c_int; L.yak_ch_get.argtypes = [P(ChT), C.c_uint64]
    L.yak_ch_inc.restype = C.c_int; L.yak_ch_inc.argtypes = [P(ChT), C.c_uint64]
    L.yak_ch_clear.argtypes = [P(ChT), C.c_int]
    L.yak_ch_shrink.argtypes = [P(ChT), C.c_int, C.c_int, C.c_int]
    L.yak_ch_hist.argtypes = [P(ChT), P(C.c_int64), C.c_int]
    L.yak_ch_dump.restype = C.c_int; L.yak_ch_dump.argtypes = [P(ChT), C.c_char_p]
    L.yak_ch_restore.restype = P(ChT); L.yak_ch_restore.argtypes = [C.c_char_p]
    L.yak_count.restype = P(ChT); L.yak_count.argtypes = [C.c_char_p, P(CoptT), P(ChT)]
    L.yakamd_count_hpc.restype = P(ChT); L.yakamd_count_hpc.argtypes = [C.c_char_p, P(CoptT), P(ChT)]
    L.yakamd_ch_set_hpc.restype = C.c_int; L.yakamd_ch_set_hpc.argtypes = [P(ChT), C.c_int]
    L.yakamd_ch_hpc.restype = C.c_int; L.yakamd_ch_hpc.argtypes = [P(ChT)]
    L.yakamd_hpc_dev.restype = C.c_int64
    L.yakamd_hpc_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.yakamd_hpc_packed_dev.restype = C.c_int64; L.yakamd_hpc_packed_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.yakamd_hpc_host.restype = C.c_int64; L.yakamd_hpc_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.yak_bf_init.restype = C.c_void_p; L.yak_bf_init.argtypes = [C.c_int, C.c_int]
    L.yak_bf_insert.restype = C.c_int; L.yak_bf_insert.argtypes = [C.c_void_p, C.c_uint64]
    L.yak_bf_destroy.argtypes = [C.c_void_p]
    L.yakamd_device_count.restype = C.c_int
    L.yakamd_last_error.restype = C.c_char_p
    L.yakamd_set_shard.restype = C.c_int; L.yakamd_set_shard.argtypes = [P(ChT), C.c_int, C.c_int]
    L.yakamd_pass_begin.restype = C.c_int; L.yakamd_pass_begin.argtypes = [P(ChT), C.c_int]
    L.yakamd_feed_bases_dev.restype = C.c_int
    L.yakamd_feed_bases_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_uint64]
    L.yakamd_packed_bytes.restype = C.c_int64
    L.yakamd_packed_bytes.argtypes = [C.c_int64]
    L.yakamd_pack_bases_host.restype = None
    L.yakamd_pack_bases_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.yakamd_feed_packed_host.restype = C.c_int
    L.yakamd_feed_packed_host.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_uint64]
    L.yakamd_feed_packed_pieces_host.restype = C.c_int
    L.yakamd_feed_packed_pieces_host.argtypes = [P(ChT), C.c_int, P(C.c_void_p), P(C.c_void_p), P(C.c_int64), C.c_uint64]
    L.yakamd_feed_packed_dev.restype = C.c_int
    L.yakamd_feed_packed_dev.argtypes = [P(ChT), C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64]
    L.yakamd_pack_bases_dev.restype = C.c_int
    L.yakamd_pack_bases_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.yakamd_feed_bases_host.restype = C.c_int
    L.yakamd_feed_bases_host.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_uint64]
    L.yakamd_feed_hashed_dev.restype = C.c_int
    L.yakamd_feed_hashed_dev.argtypes = [P(ChT), C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64]
    L.yakamd_pass_end.restype = C.c_int64; L.yakamd_pass_end.argtypes = [P(ChT)]
    L.yakamd_extract_dev.restype = C.c_int64
    L.yakamd_extract_dev.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.yakamd_sync_host.restype = C.c_int; L.yakamd_sync_host.argtypes = [P(ChT)]
    L.yakamd_dump_mem.restype = C.c_int64
    L.yakamd_dump_mem.argtypes = [P(ChT), P(P(C.c_uint8))]
    L.yakamd_dump_range_mem.restype = C.c_int64
    L.yakamd_dump_range_mem.argtypes = [P(ChT), C.c_int, C.c_int, P(P(C.c_uint8))]
    L.yakamd_yak_header.restype = C.c_int; L.yakamd_yak_header.argtypes = [C.c_char_p, P(C.c_int), P(C.c_int)]
    L.yakamd_peak_bytes.restype = C.c_int64; L.yakamd_peak_bytes.argtypes = [C.c_int, C.c_int]
    L.yakamd_last_sweeps.restype = C.c_int; L.yakamd_last_sweeps.argtypes = []
    L.yakamd_pool_report.restype = None; L.yakamd_pool_report.argtypes = [C.c_char_p]
    L.yakamd_subtable.restype = C.c_int
    L.yakamd_subtable.argtypes = [P(ChT), C.c_int, P(C.c_uint32), P(C.c_uint32)]
    L.yakamd_get_stats.restype = C.c_int; L.yakamd_get_stats.argtypes = [P(ChT), P(StatsT)]
    L.yakamd_partition_dev.restype = C.c_int64
    L.yakamd_partition_dev.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, P(C.c_uint64)]
    L.yakamd_feed_partitioned_dev.restype = C.c_int
    L.yakamd_feed_partitioned_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, P(C.c_uint64), C.c_uint64, C.c_uint64]
    L.yakamd_feed_partitioned_lent_dev.restype = C.c_int
    L.yakamd_feed_partitioned_lent_dev.argtypes = L.yakamd_feed_partitioned_dev.argtypes
    L.yakamd_tagged_ok.restype = C.c_int; L.yakamd_tagged_ok.argtypes = [C.c_int, C.c_int]
    L.yakamd_partition_tagged_dev.restype = C.c_int64
    L.yakamd_partition_tagged_dev.argtypes = L.yakamd_partition_dev.argtypes
    L.yakamd_feed_partitioned_tagged_dev.restype = C.c_int
    L.yakamd_feed_partitioned_tagged_dev.argtypes = list(L.yakamd_feed_partitioned_dev.argtypes) + [C.c_int]
    L.yakamd_partition_hashes_dev.restype = C.c_int64
    L.yakamd_partition_hashes_dev.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, P(C.c_uint64)]
    L.yakamd_count_partitioned_dev.restype = C.c_int
    L.yakamd_count_partitioned_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, P(C.c_uint64)]
    L.yakamd_count_hashes_dev.restype = C.c_int
    L.yakamd_count_hashes_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64]
    L.yakamd_host_image.restype = C.c_int64
    L.yakamd_host_image.argtypes = [C.c_char_p, C.c_int, C.c_int, P(C.c_void_p)]
    L.yakamd_host_image_packed.restype = C.c_int64
    L.yakamd_host_image_packed.argtypes = [C.c_char_p, C.c_int, P(C.c_void_p)]
    L.yakamd_test_set.restype = None
    L.yakamd_test_set.argtypes = [C.c_char_p, C.c_int64]
    L.yakamd_test_reset.restype = None
    L.yakamd_test_reset.argtypes = []
    L.yakamd_tally_names.restype = C.c_int
    L.yakamd_tally_names.argtypes = [P(P(C.c_char_p))]
    L.yakamd_tally_read.restype = None
    L.yakamd_tally_read.argtypes = [P(C.c_uint64), C.c_int]
    L.yakamd_tally_reset.restype = None
    L.yakamd_tally_reset.argtypes = []
    L.yakamd_gz_tune.restype = None
    L.yakamd_gz_tune.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.yakamd_gz_inflate.restype = C.c_int64
    L.yakamd_gz_inflate.argtypes = [C.c_char_p, C.c_int, P(C.c_void_p)]
    L.yak_ch_setcnt.argtypes = [P(ChT), C.c_int, C.c_int]
    L.yak_ch_restore_core.restype = P(ChT)
    L.yak_qv_solve.restype = C.c_int
    L.yak_qv_solve.argtypes = [P(C.c_int64), P(C.c_int64), C.c_int, C.c_double, P(QstatT)]
    L.yak_ch_tighten.argtypes = [P(ChT)]
    L.yak_ch_merge.argtypes = [P(ChT), P(ChT), C.c_int, C.c_int, C.c_int, C.c_int]
    L.yak_ch_subtract.argtypes = [P(ChT), P(ChT), C.c_int]
    L.yak_ch_isec.argtypes = [P(ChT), P(ChT), C.c_int]
    L.yak_recount.restype = None; L.yak_recount.argtypes = [C.c_char_p, P(ChT)]
    L.yak_qopt_init.argtypes = [P(QoptT)]
    L.yak_qv.restype = None; L.yak_qv.argtypes = [P(QoptT), C.c_char_p, P(ChT), P(C.c_int64)]
    L.yakamd_lookup_dev.restype = C.c_int; L.yakamd_lookup_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_void_p]
    L.yakamd_retain_input.restype = C.c_int; L.yakamd_retain_input.argtypes = [P(ChT), C.c_int]
    L.yakamd_count_retained.restype = C.c_int; L.yakamd_count_retained.argtypes = [P(ChT)]
    L.yakamd_retained_instances.restype = C.c_int64; L.yakamd_retained_instances.argtypes = [P(ChT)]
    L.yakamd_count_multi_dev.restype = P(ChT)
    L.yakamd_count_multi_dev.argtypes = [P(CoptT), P(ChT), C.c_int, P(C.c_int), C.c_int, P(C.c_void_p), P(C.c_int64), P(C.c_int)]
    L.yakamd_qv_reduce_dev.restype = C.c_int
    L.yakamd_qv_reduce_dev.argtypes = [P(ChT), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    L.yakamd_host_alloc.restype = C.c_void_p; L.yakamd_host_alloc.argtypes = [C.c_size_t]
    L.yakamd_host_free.argtypes = [C.c_void_p]
    L.yakamd_device_sync.restype = C.c_int
    L.yakamd_mem_info.restype = C.c_int; L.yakamd_mem_info.argtypes = [P(C.c_size_t), P(C.c_size_t)]
    L.yakamd_dev_alloc.restype = C.c_void_p; L.yakamd_dev_alloc.argtypes = [C.c_size_t]
    L.yakamd_dev_free.argtypes = [C.c_void_p]
    L.yakamd_memcpy_h2d.restype = C.c_int; L.yakamd_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.yakamd_memcpy_d2h.restype = C.c_int; L.yakamd_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.yakamd_triobin_lookup_dev.restype = C.c_int
    L.yakamd_triobin_lookup_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_void_p]
    L.yakamd_triobin_reduce_dev.restype = C.c_int
    L.yakamd_triobin_reduce_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.yakamd_tbopt_init.restype = None; L.yakamd_tbopt_init.argtypes = [P(TboptT)]
    L.yakamd_triobin.restype = C.c_int; L.yakamd_triobin.argtypes = [P(TboptT), P(ChT), C.c_char_p, C.c_char_p]
    L.yakamd_trioeval_reduce_dev.restype = C.c_int
    L.yakamd_trioeval_reduce_dev.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                             P(C.c_void_p), P(C.c_int64), C.c_void_p]
    L.yakamd_teopt_init.restype = None; L.yakamd_teopt_init.argtypes = [P(TeoptT)]
    L.yakamd_trioeval.restype = C.c_int; L.yakamd_trioeval.argtypes = [P(TeoptT), P(ChT), C.c_char_p, C.c_char_p]
    L.yakamd_inspect_dev.restype = C.c_int
    L.yakamd_inspect_dev.argtypes = [P(ChT), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]
    L.yakamd_inopt_init.restype = None; L.yakamd_inopt_init.argtypes = [P(InoptT)]
    L.yakamd_inspect.restype = C.c_int; L.yakamd_inspect.argtypes = [P(InoptT), C.c_char_p, C.c_char_p, C.c_char_p]
    L.yakamd_inspect_tables.restype = C.c_int; L.yakamd_inspect_tables.argtypes = [P(ChT), P(ChT), C.c_int, P(C.c_int64)]
    L.yakamd_chkerr_lookup_dev.restype = C.c_int
    L.yakamd_chkerr_lookup_dev.argtypes = [P(ChT), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.yakamd_chkerr_streaks_dev.restype = C.c_int
    L.yakamd_chkerr_streaks_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, P(C.c_void_p), P(C.c_int64), C.c_void_p]
    L.yakamd_ceopt_init.restype = None; L.yakamd_ceopt_init.argtypes = [P(CeoptT)]
    L.yakamd_chkerr.restype = C.c_int; L.yakamd_chkerr.argtypes = [P(CeoptT), P(ChT), C.c_char_p, C.c_char_p]
    L.yakamd_sexchr_reduce_dev.restype = C.c_int
    L.yakamd_sexchr_reduce_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.yakamd_scopt_init.restype = None; L.yakamd_scopt_init.argtypes = [P(ScoptT)]
    L.yakamd_sexchr.restype = C.c_int; L.yakamd_sexchr.argtypes = [P(ScoptT), P(ChT), C.c_char_p, C.c_char_p, C.c_char_p]
    L.yakamd_kmers_dev.restype = C.c_int64
    L.yakamd_kmers_dev.argtypes = [P(ChT), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    L.yakamd_print_dev.restype = C.c_int64
    L.yakamd_print_dev.argtypes = [P(ChT), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.yakamd_propt_init.restype = None; L.yakamd_propt_init.argtypes = [P(PropT)]
    L.yakamd_print.restype = C.c_int; L.yakamd_print.argtypes = [P(PropT), P(ChT), C.c_char_p]
    L.yakamd_host_syncs.restype = C.c_int64; L.yakamd_host_syncs.argtypes = []
    L.yak_ch_tighten.restype = None; L.yak_ch_tighten.argtypes = [P(ChT)]
    L.yakamd_ch_sum.restype = C.c_int; L.yakamd_ch_sum.argtypes = [P(ChT), P(ChT), C.c_int]
    L.yakamd_depth_reduce_dev.restype = C.c_int
    L.yakamd_depth_reduce_dev.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.yakamd_dpopt_init.restype = None; L.yakamd_dpopt_init.argtypes = [P(DpoptT)]
    L.yakamd_depth.restype = C.c_int; L.yakamd_depth.argtypes = [P(DpoptT), P(ChT), C.c_char_p, C.c_char_p]
    L.yakamd_cover_dev.restype = C.c_int
    L.yakamd_cover_dev.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]
    L.yakamd_cvopt_init.restype = None; L.yakamd_cvopt_init.argtypes = [P(CvoptT)]
    L.yakamd_cover.restype = C.c_int; L.yakamd_cover.argtypes = [P(CvoptT), P(ChT), C.c_char_p, C.c_char_p]
    L.yakamd_hetmers_dev.restype = C.c_int; L.yakamd_hetmers_dev.argtypes = [P(ChT), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.yakamd_hetmer_pairs_dev.restype = C.c_int64; L.yakamd_hetmer_pairs_dev.argtypes = [P(ChT), C.c_int, C.c_void_p, C.c_int64]
    L.yakamd_hmopt_init.restype = None; L.yakamd_hmopt_init.argtypes = [P(HmoptT)]
    L.yakamd_hetmers.restype = C.c_int; L.yakamd_hetmers.argtypes = [P(HmoptT), P(ChT), C.c_char_p]
    L.yakamd_graph_open.restype = C.c_void_p; L.yakamd_graph_open.argtypes = [P(ChT), C.c_int]
    L.yakamd_graph_stats.restype = C.c_int; L.yakamd_graph_stats.argtypes = [C.c_void_p, P(GstatT)]
    L.yakamd_graph_nodes_dev.restype = C.c_int64; L.yakamd_graph_nodes_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.yakamd_graph_close.restype = None; L.yakamd_graph_close.argtypes = [C.c_void_p]
    L.yakamd_graph_open_ms.restype = None; L.yakamd_graph_open_ms.argtypes = [C.c_void_p, P(C.c_double)]
    L.yakamd_ugopt_init.restype = None; L.yakamd_ugopt_init.argtypes = [P(UgoptT)]
    L.yakamd_unitigs_ms.restype = None; L.yakamd_unitigs_ms.argtypes = [P(C.c_double)]
    L.yakamd_unitigs.restype = C.c_int; L.yakamd_unitigs.argtypes = [P(UgoptT), P(ChT), C.c_char_p]
    _lib = L
    return L


def _err():
    return (lib().yakamd_last_error() or b"").decode()


def _output_of(name, call):
    """what a command wrote: `call(path)` is the C call writing to `path`; a non-zero return raises with the library's error text"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, name + ".txt")
        if call(out.encode()) != 0:
            raise RuntimeError(name + " failed: " + _err())
        with open(out, "rb") as f:
            return f.read()


class Table:
    """Thin owner of a ``yak_ch_t *`` created through the C ABI."""

    def __init__(self, k=31, pre=10, n_hash=4, bf_shift=0, ptr=None):
        self.L = lib()
        self.h = ptr if ptr is not None else self.L.yak_ch_init(k, pre, n_hash, bf_shift)
        if not self.h:
            raise RuntimeError("yak_ch_init failed: " + _err())

    # -- reference protocol pieces ---------------------------------------------------------
    def count_pass(self, create_new, feeds, same_input=False):
        """one pass: feeds = iterable of (device_ptr, n_bytes, t0).  same_input (create_new = 0 only): the feeds are the ones of
        the create_new pass before -- the records that pass retained (yakamd_retain_input) are counted instead, if there are any"""
        if self.L.yakamd_pass_begin(self.h, create_new) != 0:
            raise RuntimeError(_err())
        r = self.L.yakamd_count_retained(self.h) if (same_input and not create_new) else 1
        if r < 0:
            raise RuntimeError(_err())
        for ptr, n, t0 in (feeds if r else ()):
            if self.L.yakamd_feed_bases_dev(self.h, ptr, n, t0) != 0:
                raise RuntimeError(_err())
        n_ins = self.L.yakamd_pass_end(self.h)
        if n_ins < 0:
            raise RuntimeError(_err())
        self.h.contents.tot += n_ins
        return n_ins

    def count_pass_packed(self, create_new, feeds, same_input=False):
        """one pass over packed images: feeds = iterable of (codes_ptr, valid_ptr, n_bases, t0) (yakamd_feed_packed_dev)"""
        if self.L.yakamd_pass_begin(self.h, create_new) != 0:
            raise RuntimeError(_err())
        r = self.L.yakamd_count_retained(self.h) if (same_input and not create_new) else 1
        if r < 0:
            raise RuntimeError(_err())
        for codes, valid, n, t0 in (feeds if r else ()):
            if self.L.yakamd_feed_packed_dev(self.h, codes, valid, n, t0) != 0:
                raise RuntimeError(_err())
        n_ins = self.L.yakamd_pass_end(self.h)
        if n_ins < 0:
            raise RuntimeError(_err())
        self.h.contents.tot += n_ins
        return n_ins

    def count_pass_packed_host(self, create_new, pieces, as_one=False):
        """one pass over pieces of the stream, each packed on the host (pack_bases_host) and fed from host memory: pieces = iterable of (ascii bytes, t0);
        as_one: all of them in ONE feed (yakamd_feed_packed_pieces_host), every piece taken to end at a multiple of 32 positions"""
        if self.L.yakamd_pass_begin(self.h, create_new) != 0:
            raise RuntimeError(_err())
        if as_one:
            pieces = list(pieces)
            pk = [pack_bases_host(buf) for buf, _ in pieces]
            nw = [(len(buf) + 31) // 32 for buf, _ in pieces]
            keep = [C.create_string_buffer(x, len(x)) for x in pk]
            codes = (C.c_void_p * len(pk))(*[C.addressof(k) for k in keep])
            valid = (C.c_void_p * len(pk))(*[C.addressof(k) + ((8 * w + 15) & ~15) for k, w in zip(keep, nw)])
            if self.L.yakamd_feed_packed_pieces_host(self.h, len(pk), codes, valid, (C.c_int64 * len(pk))(*nw), pieces[0][1] if pieces else 0) != 0:
                raise RuntimeError(_err())
            pieces = ()
        for buf, t0 in pieces:
            pk = pack_bases_host(buf)
            if self.L.yakamd_feed_packed_host(self.h, pk, len(buf), t0) != 0:
                raise RuntimeError(_err())
        n_ins = self.L.yakamd_pass_end(self.h)
        if n_ins < 0:
            raise RuntimeError(_err())
        self.h.contents.tot += n_ins
        return n_ins

    def count_pass_host(self, create_new, buf, t0=0):
        if self.L.yakamd_pass_begin(self.h, create_new) != 0:
            raise RuntimeError(_err())
        cbuf = (C.c_char * len(buf)).from_buffer_copy(buf)
        if self.L.yakamd_feed_bases_host(self.h, cbuf, len(buf), t0) != 0:
            raise RuntimeError(_err())
        n_ins = self.L.yakamd_pass_end(self.h)
        if n_ins < 0:
            raise RuntimeError(_err())
        self.h.contents.tot += n_ins
        return n_ins

    def destroy_bf(self):
        self.L.yak_ch_destroy_bf(self.h)

    def clear(self):
        self.L.yak_ch_clear(self.h, 1)

    def shrink(self, lo, hi):
        self.L.yak_ch_shrink(self.h, lo, hi, 1)

    @property
    def tot(self):
        return self.h.contents.tot

    def stats(self):
        st = StatsT()
        self.L.yakamd_get_stats(self.h, C.byref(st))
        return {f: getattr(st, f) for f, _ in StatsT._fields_}

    def dump_bytes(self):
        out = C.POINTER(C.c_uint8)()
        n = self.L.yakamd_dump_mem(self.h, C.byref(out))
        if n < 0:
            raise RuntimeError(_err())
        addr = C.cast(out, C.c_void_p).value
        data = bytes((C.c_char * n).from_address(addr))          # C.string_at takes a C int: .yak files pass 2 GB
        C.CDLL(None).free(out)
        return data

    def dump_md5(self):
        """md5 of the .yak bytes without a second copy of them (multi-GB tables)"""
        import hashlib
        out = C.POINTER(C.c_uint8)()
        n = self.L.yakamd_dump_mem(self.h, C.byref(out))
        if n < 0:
            raise RuntimeError(_err())
        addr = C.cast(out, C.c_void_p).value
        h = hashlib.md5()
        step = 1 << 28
        for o in range(0, n, step):
            h.update((C.c_char * min(step, n - o)).from_address(addr + o))
        C.CDLL(None).free(out)
        return h.hexdigest(), n

    def range_md5(self, lo, hi):
        """md5 and size of the bytes of sub-tables [lo, hi) ({capacity, size, keys in slot order} each, no header): one rank's share of the .yak file"""
        import hashlib
        out = C.POINTER(C.c_uint8)()
        n = self.L.yakamd_dump_range_mem(self.h, lo, hi, C.byref(out))
        if n < 0:
            raise RuntimeError(_err())
        addr = C.cast(out, C.c_void_p).value
        h = hashlib.md5()
        step = 1 << 28
        for o in range(0, n, step):
            h.update((C.c_char * min(step, n - o)).from_address(addr + o))
        C.CDLL(None).free(out)
        return h.hexdigest(), n

    def hetmers(self, min_cnt=1):
        """the het-mer pairs of the table (yakamd_hetmers_dev): (J as a dict {(lo, hi): pairs with those two counts}, n_group as a list of 5,
        [s] = groups of s k-mers that differ in the middle base alone)"""
        import struct
        n = 1024 * 1024 * 8 + 64                                # J, then the five group counts
        d = self.L.yakamd_dev_alloc(n)
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + _err())
        try:
            if self.L.yakamd_memcpy_h2d(d, bytes(n), n) != 0 or self.L.yakamd_hetmers_dev(self.h, min_cnt, d, d + 1024 * 1024 * 8, None) != 0:
                raise RuntimeError("yakamd_hetmers_dev failed: " + _err())
            buf = C.create_string_buffer(n)
            if self.L.yakamd_memcpy_d2h(buf, d, n) != 0:
                raise RuntimeError(_err())
        finally:
            self.L.yakamd_dev_free(d)
        raw = buf.raw
        group = list(struct.unpack_from("<5Q", raw, 1024 * 1024 * 8))
        J = {}
        for lo in range(1024):
            row = raw[lo * 8192:(lo + 1) * 8192]
            if any(row):
                J.update({(lo, hi): v for hi, v in enumerate(struct.unpack("<1024Q", row)) if v})
        return J, group

    def hetmer_pairs(self, min_cnt=1):
        """the het-mer pairs themselves (yakamd_hetmer_pairs_dev): [(x, y, cx, cy)] with x < y, in the table's listing order of x"""
        n = self.L.yakamd_hetmer_pairs_dev(self.h, min_cnt, None, 0)
        if n < 0:
            raise RuntimeError("yakamd_hetmer_pairs_dev failed: " + _err())
        if n == 0:
            return []
        d = self.L.yakamd_dev_alloc(n * C.sizeof(HetpairT))
        if not d:
            raise RuntimeError("yakamd_dev_alloc failed: " + _err())
        try:
            if self.L.yakamd_hetmer_pairs_dev(self.h, min_cnt, d, n) != n:
                raise RuntimeError("yakamd_hetmer_pairs_dev failed: " + _err())
            recs = (HetpairT * n)()
            if self.L.yakamd_memcpy_d2h(recs, d, n * C.sizeof(HetpairT)) != 0:
                raise RuntimeError(_err())
        finally:
            self.L.yakamd_dev_free(d)
        return [(r.x, r.y, r.cx, r.cy) for r in recs]

    def graph_stats(self, min_cnt=1):
        """the tallies of the table's de Bruijn graph (yakamd_graph_open + yakamd_graph_stats): a dict of n_key, n_node, n_arc, n_linked_side and
        deg, deg[l][r] = nodes of l left and r right edges"""
        g = self.L.yakamd_graph_open(self.h, min_cnt)
        if not g:
            raise RuntimeError("yakamd_graph_open failed: " + _err())
        try:
            st = GstatT()
            if self.L.yakamd_graph_stats(g, C.byref(st)) != 0:
                raise RuntimeError("yakamd_graph_stats failed: " + _err())
        finally:
            self.L.yakamd_graph_close(g)
        return dict(n_key=st.n_key, n_node=st.n_node, n_arc=st.n_arc, n_linked_side=st.n_linked_side, deg=[[st.deg[l][r] for r in range(5)] for l in range(5)])

    def graph_nodes(self, min_cnt=1, sub_lo=0, sub_hi=None):
        """the graph's records of the stored keys of sub-tables [sub_lo, sub_hi) in listing order (yakamd_graph_nodes_dev): [(x, link_r, link_l, count,
        edges)], a link = the global listing index of the linked node << 1 | its facing side, or 2^64 - 1"""
        sub_hi = (1 << self.h.contents.pre) if sub_hi is None else sub_hi
        g = self.L.yakamd_graph_open(self.h, min_cnt)
        if not g:
            raise RuntimeError("yakamd_graph_open failed: " + _err())
        d = None
        try:
            n = self.L.yakamd_graph_nodes_dev(g, sub_lo, sub_hi, None, 0)
            if n < 0:
                raise RuntimeError("yakamd_graph_nodes_dev failed: " + _err())
            if n == 0:
                return []
            d = self.L.yakamd_dev_alloc(n * C.sizeof(GnodeT))
            if not d:
                raise RuntimeError("yakamd_dev_alloc failed: " + _err())
            if self.L.yakamd_graph_nodes_dev(g, sub_lo, sub_hi, d, n) != n:
                raise RuntimeError("yakamd_graph_nodes_dev failed: " + _err())
            recs = (GnodeT * n)()
            if self.L.yakamd_memcpy_d2h(recs, d, n * C.sizeof(GnodeT)) != 0:
                raise RuntimeError(_err())
        finally:
            if d:
                self.L.yakamd_dev_free(d)
            self.L.yakamd_graph_close(g)
        return [(r.x, r.link[0], r.link[1], r.count, r.edges) for r in recs]

    def subtable(self, i):
        cap, size = C.c_uint32(), C.c_uint32()
        self.L.yakamd_subtable(self.h, i, C.byref(cap), C.byref(size))
        return cap.value, size.value

    def close(self):
        if self.h:
            self.L.yak_ch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def count_protocol_host(buf1, k=31, pre=10, n_hash=4, bf_shift=0, buf2=None):
    """`yak count` protocol of reference main.c:53-60 on in-memory base images -> .yak bytes"""
    t = Table(k, pre, n_hash, bf_shift)
    try:
        t.count_pass_host(1, buf1)
        if bf_shift > 0:
            t.destroy_bf()
            t.clear()
            t.count_pass_host(0, buf2 if buf2 is not None else buf1)
            t.shrink(2, 1023)
        return t.dump_bytes(), t.tot
    finally:
        t.close()


def qv_counts(table_fn, seq_fn, min_len=0, min_frac=0.5, chunk=1000000000):
    """`yak qv` counting step through the C ABI (yak_ch_restore + yak_qv): the 1024-bin histogram of
    table counts over the k-mers of the accepted sequences"""
    L = lib()
    h = L.yak_ch_restore(table_fn.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    o = QoptT()
    L.yak_qopt_init(C.byref(o))
    o.min_len, o.min_frac, o.chunk_size = min_len, min_frac, chunk
    cnt = (C.c_int64 * 1024)()
    L.yak_qv(C.byref(o), seq_fn.encode(), h, cnt)
    L.yak_ch_destroy(h)
    return list(cnt)


def triobin_table(pat_yak, mat_yak, min_cnt=2, mid_cnt=5):
    """the table of `yak triobin` (reference triobin.c:187-188): both parents' classes in one table"""
    L = lib()
    h = L.yak_ch_restore_core(None, pat_yak.encode(), 2, C.c_int(min_cnt), C.c_int(mid_cnt))       # YAK_LOAD_TRIOBIN1
    if h:
        h = L.yak_ch_restore_core(h, mat_yak.encode(), 3, C.c_int(min_cnt), C.c_int(mid_cnt))     # YAK_LOAD_TRIOBIN2
    if not h:
        raise RuntimeError("yak_ch_restore_core (TRIOBIN) failed: " + _err())
    return h


def triobin(pat_yak, mat_yak, seq_fn, min_cnt=2, mid_cnt=5, ratio=0.33, print_diff=False, chunk=None):
    """`yak triobin` through the C ABI (two TRIOBIN loads + yakamd_triobin): the bytes the reference writes with -t1"""
    L = lib()
    h = triobin_table(pat_yak, mat_yak, min_cnt, mid_cnt)
    try:
        o = TboptT()
        L.yakamd_tbopt_init(C.byref(o))
        o.ratio_thres, o.print_diff = ratio, int(bool(print_diff))
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_triobin", lambda out: L.yakamd_triobin(C.byref(o), h, seq_fn.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def trioeval(pat_yak, mat_yak, seq_fn, min_cnt=2, mid_cnt=5, min_n=2, print_err=False, print_frag=True, chunk=None):
    """`yak trioeval` through the C ABI (two TRIOBIN loads + yakamd_trioeval): the bytes the reference writes to stdout with -t1"""
    L = lib()
    h = triobin_table(pat_yak, mat_yak, min_cnt, mid_cnt)
    try:
        o = TeoptT()
        L.yakamd_teopt_init(C.byref(o))
        o.min_n, o.print_err, o.print_frag = min_n, int(bool(print_err)), int(bool(print_frag))
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_trioeval", lambda out: L.yakamd_trioeval(C.byref(o), h, seq_fn.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def chkerr(count_yak, seq, min_cnt=3, min_streak=5, chunk=None):
    """`yak chkerr` through the C ABI (yak_ch_restore + yakamd_chkerr): the bytes the reference writes to stdout with -t1"""
    L = lib()
    h = L.yak_ch_restore(count_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    try:
        o = CeoptT()
        L.yakamd_ceopt_init(C.byref(o))
        o.min_cnt, o.min_streak = min_cnt, min_streak
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_chkerr", lambda out: L.yakamd_chkerr(C.byref(o), h, seq.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def depth(table_yak, seq, window=0, chunk=None):
    """`yak-amd depth` through the C ABI (yak_ch_restore + yakamd_depth): one line per sequence (window = 0) or per window of `window` k-mer
    start positions -- name, start, end, n_kmer, n_present, mean, median, max -- behind a `#` header line"""
    L = lib()
    h = L.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    try:
        o = DpoptT()
        L.yakamd_dpopt_init(C.byref(o))
        o.window = window
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_depth", lambda out: L.yakamd_depth(C.byref(o), h, seq.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def hetmers(table_yak, min_cnt=1, pairs=False, batch_keys=None):
    """`yak-amd hetmers` through the C ABI (yak_ch_restore + yakamd_hetmers): the `#hetmers` line, with `pairs` a K line per pair of k-mers that
    differ in the middle base alone, the G lines (groups of 1 .. 4 such k-mers) and a P line per non-zero bin of the pairs' two counts"""
    L = lib()
    h = L.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    try:
        o = HmoptT()
        L.yakamd_hmopt_init(C.byref(o))
        o.min_cnt, o.print_pairs = min_cnt, int(bool(pairs))
        if batch_keys is not None:
            o.batch_keys = batch_keys
        return _output_of("yakamd_hetmers", lambda out: L.yakamd_hetmers(C.byref(o), h, out))
    finally:
        L.yak_ch_destroy(h)


def unitigs(table_yak, min_cnt=1, stats_only=False, threads=None, batch_keys=None):
    """`yak-amd unitigs` through the C ABI (yak_ch_restore + yakamd_unitigs): the unitigs of the de Bruijn graph that the table's k-mers with a count
    of at least min_cnt span, as FASTA (open unitigs first, then cycles), or with stats_only the `#unitigs`, N, D and U lines"""
    L = lib()
    h = L.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    try:
        o = UgoptT()
        L.yakamd_ugopt_init(C.byref(o))
        o.min_cnt, o.stats_only = min_cnt, int(bool(stats_only))
        if threads is not None:
            o.n_threads = threads
        if batch_keys is not None:
            o.batch_keys = batch_keys
        return _output_of("yakamd_unitigs", lambda out: L.yakamd_unitigs(C.byref(o), h, out))
    finally:
        L.yak_ch_destroy(h)


def cover(table_yak, seq, lo=1, hi=1023, intervals=False, mask=None, min_frac=0.0, min_hit=0, invert=False, chunk=None):
    """`yak-amd cover` through the C ABI (yak_ch_restore + yakamd_cover): which bases of every sequence lie inside k-mers whose count in the table
    is in [lo, hi] -- the `#cover` line, one S line per selected sequence (with `intervals` its B lines behind it) and the T line; with mask =
    "none", "soft" or "hard" the selected sequences as FASTA instead, covered bases as they are, in lower case or as N"""
    L = lib()
    masks = {None: -1, "none": 0, "soft": 1, "hard": 2}
    if mask not in masks:
        raise ValueError("mask is None, 'none', 'soft' or 'hard'")
    h = L.yak_ch_restore(table_yak.encode())
    if not h:
        raise RuntimeError("yak_ch_restore failed: " + _err())
    try:
        o = CvoptT()
        L.yakamd_cvopt_init(C.byref(o))
        o.lo, o.hi, o.intervals, o.mask, o.invert, o.min_hit, o.min_frac = lo, hi, int(bool(intervals)), masks[mask], int(bool(invert)), min_hit, min_frac
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_cover", lambda out: L.yakamd_cover(C.byref(o), h, seq.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def yak_header(fn):
    """(k, pre) of a .yak file's header (yakamd_yak_header); a file that cannot be opened raises as open() does"""
    with open(fn, "rb"):
        pass
    k, pre = C.c_int(), C.c_int()
    if lib().yakamd_yak_header(os.fsencode(fn), C.byref(k), C.byref(pre)) != 0:
        raise ValueError("%s: not a .yak file" % fn)
    return k.value, pre.value


def sexchr_table(y, x, par):
    """the table of `yak sexchr` (reference sexchr.c:116-118): flags 1 | 2 | 4 from the chrY, chrX and PAR tables, which must agree on k and pre"""
    hdr = [yak_header(f) for f in (y, x, par)]
    if len(set(hdr)) != 1:
        raise ValueError("sexchr: the three tables differ in k or pre: %s" % hdr)
    L = lib()
    h = L.yak_ch_restore_core(None, y.encode(), 4)            # YAK_LOAD_SEXCHR1
    if h:
        h = L.yak_ch_restore_core(h, x.encode(), 5)           # YAK_LOAD_SEXCHR2
    if h:
        h = L.yak_ch_restore_core(h, par.encode(), 6)         # YAK_LOAD_SEXCHR3
    if not h:
        raise RuntimeError("yak_ch_restore_core (SEXCHR) failed: " + _err())
    return h


def sexchr(y, x, par, hap1, hap2, chunk=None):
    """`yak sexchr` through the C ABI (three SEXCHR loads + yakamd_sexchr): the bytes the reference writes to stdout with -t1"""
    L = lib()
    h = sexchr_table(y, x, par)
    try:
        o = ScoptT()
        L.yakamd_scopt_init(C.byref(o))
        if chunk is not None:
            o.chunk_size = chunk
        return _output_of("yakamd_sexchr", lambda out: L.yakamd_sexchr(C.byref(o), h, hap1.encode(), hap2.encode(), out))
    finally:
        L.yak_ch_destroy(h)


def inspect(in1, in2=None, max_cnt=20, ref_probe=False, batch_keys=None):
    """`yak inspect` through the C ABI (yakamd_inspect): the bytes the reference's inspect.c writes to stdout (ref_probe: its probe of in2)"""
    L = lib()
    o = InoptT()
    L.yakamd_inopt_init(C.byref(o))
    o.max_cnt, o.ref_probe = max_cnt, int(bool(ref_probe))
    if batch_keys is not None:
        o.batch_keys = batch_keys
    return _output_of("yakamd_inspect", lambda out: L.yakamd_inspect(C.byref(o), in1.encode(), in2.encode() if in2 else None, out))


def inspect_tables(a, b=None, ref_probe=False):
    """the joint spectrum of two resident tables (``yak_ch_t *`` or Table; b None: one table) as a 1024 x 1024 int64 numpy array, row = count in a"""
    import numpy as np
    L = lib()
    J = np.zeros((1024, 1024), np.int64)
    ha = a.h if isinstance(a, Table) else a
    hb = (b.h if isinstance(b, Table) else b) if b is not None else None
    if L.yakamd_inspect_tables(ha, hb, int(bool(ref_probe)), J.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise RuntimeError("yakamd_inspect_tables failed: " + _err())
    return J


def print_table(h, counts=False, batch_bytes=None):
    """yakamd_print of a resident table (a ``yak_ch_t *``), as it is: the bytes `yak print [-c]` writes"""
    L = lib()
    o = PropT()
    L.yakamd_propt_init(C.byref(o))
    o.with_counts = int(bool(counts))
    if batch_bytes is not None:
        o.batch_bytes = batch_bytes
    return _output_of("yakamd_print", lambda out: L.yakamd_print(C.byref(o), h, out))


def print_kmers(table_fn, counts=False, batch_bytes=None, tighten=True):
    """`yak print [-c]` through the C ABI (yak_ch_restore, yak_ch_tighten, yakamd_print): the bytes the reference writes to stdout"""
    L = lib()
    h = L.yak_ch_restore(table_fn.encode())
    if not h:
        raise RuntimeError("print: cannot load " + table_fn)
    try:
        if tighten:
            L.yak_ch_tighten(h)
        return print_table(h, counts, batch_bytes)
    finally:
        L.yak_ch_destroy(h)


def kmers(table, sub_lo=0, sub_hi=None):
    """the k-mers of sub-tables [sub_lo, sub_hi) of a .yak file (restored, not tightened) or of a resident table (``yak_ch_t *``), in
    yak_ch_getseq's order (yakamd_kmers_dev): (numpy uint64 k-mers, numpy uint16 counts)"""
    import numpy as np
    L = lib()
    own = isinstance(table, str)
    h = L.yak_ch_restore(table.encode()) if own else table
    if not h:
        raise RuntimeError("kmers: cannot load %s" % (table,))
    dx = dc = None
    try:
        hi = (1 << h.contents.pre) if sub_hi is None else sub_hi
        n = L.yakamd_kmers_dev(h, sub_lo, hi, None, None, 0)
        if n < 0:
            raise RuntimeError("yakamd_kmers_dev failed: " + _err())
        x, c = np.zeros(n, np.uint64), np.zeros(n, np.uint16)
        if n:
            dx, dc = L.yakamd_dev_alloc(n * 8), L.yakamd_dev_alloc(n * 2)
            if not dx or not dc or L.yakamd_kmers_dev(h, sub_lo, hi, dx, dc, n) != n:
                raise RuntimeError("yakamd_kmers_dev failed: " + _err())
            if L.yakamd_memcpy_d2h(x.ctypes.data, dx, n * 8) != 0 or L.yakamd_memcpy_d2h(c.ctypes.data, dc, n * 2) != 0:
                raise RuntimeError("kmers: copy back failed")
        return x, c
    finally:
        L.yakamd_dev_free(dx); L.yakamd_dev_free(dc)
        if own:
            L.yak_ch_destroy(h)


def sum_tables(paths, out=None, pre_resize=False):
    """`yak-amd sum` through the C ABI: restore the first .yak file, yakamd_ch_sum every further one into it, yak_ch_tighten.  With `out` the
    table is dumped to that path, which is returned; without it the .yak bytes are returned"""
    L = lib()
    if len(paths) < 2:
        raise ValueError("sum_tables: at least two tables")
    def restore(fn):
        h = L.yak_ch_restore(fn.encode())
        if not h:
            raise RuntimeError("sum_tables: cannot load %s (not a readable .yak file, or no MI355X)" % fn)
        return Table(ptr=h)
    t = restore(paths[0])
    try:
        for fn in paths[1:]:
            other = restore(fn)
            try:
                if L.yakamd_ch_sum(t.h, other.h, int(bool(pre_resize))) != 0:
                    raise RuntimeError("yakamd_ch_sum failed: " + _err())
            finally:
                other.close()
        L.yak_ch_tighten(t.h)
        if out is None:
            return t.dump_bytes()
        if L.yak_ch_dump(t.h, out.encode()) != 0:
            raise OSError("sum_tables: cannot write " + out)
        return out
    finally:
        t.close()


def pack_bases_host(buf):
    """the packed image of an ASCII base image (host only): code words, then -- 16-byte aligned -- validity words"""
    L = lib()
    n = len(buf)
    out = C.create_string_buffer(max(16, L.yakamd_packed_bytes(n)))
    src = (C.c_char * max(1, n)).from_buffer_copy(buf if n else b"\0")
    L.yakamd_pack_bases_host(src, n, out)
    return out.raw[:L.yakamd_packed_bytes(n)]


def gz_tune(chunk_bytes=0, min_file_bytes=-1, front_bytes=-1):
    """test hook: the gzip reader's bytes per thread and batch, the smallest file it takes, the room in front of a batch"""
    lib().yakamd_gz_tune(chunk_bytes, min_file_bytes, front_bytes)


def gz_inflate(fn, threads=4):
    """the inflated stream of gzip file `fn` as the parallel reader delivers it (host only); None if it does not take the file"""
    L = lib()
    out = C.c_void_p()
    n = L.yakamd_gz_inflate(fn.encode(), threads, C.byref(out))
    if n == -1:
        return None
    if n < 0:
        raise OSError("invalid gzip stream in " + fn + ": " + L.yakamd_last_error().decode())
    data = C.string_at(out, n)
    C.CDLL(None).free(out)
    return data


def host_image_packed(fn, min_len=0):
    """the stream yak_count() feeds for `fn` when its parser threads pack, unpacked again (host only); None if the parallel parser does not take the file"""
    L = lib()
    out = C.c_void_p()
    n = L.yakamd_host_image_packed(fn.encode(), min_len, C.byref(out))
    if n < 0:
        return None
    data = C.string_at(out, n)
    C.CDLL(None).free(out)
    return data


def host_image(fn, min_len=0, fast=True):
    """the base image yak_count() would feed for file `fn` (host only)"""
    L = lib()
    out = C.c_void_p()
    n = L.yakamd_host_image(fn.encode(), min_len, 1 if fast else 0, C.byref(out))
    if n < 0:
        raise OSError("cannot read " + fn)
    data = C.string_at(out, n)
    C.CDLL(None).free(out)
    return data


def kernels_sha16():
    """sha256 (first 16 hex digits) over the device code the library is built from (csrc/kernels.hip, kern_*.inc, yk_device.h): the counter passes under
    profiles/ carry the value they were measured on, and bench.py reports `roofline.traffic` only while it equals the value of the tree it runs from."""
    import glob, hashlib
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha256()
    for fn in sorted(glob.glob(os.path.join(d, "kern_*.inc")) + [os.path.join(d, "kernels.hip"), os.path.join(d, "yk_device.h")]):
        h.update(os.path.basename(fn).encode() + b"\0")
        h.update(open(fn, "rb").read())
    return h.hexdigest()[:16]
