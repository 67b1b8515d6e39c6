"""ctypes binding of include/pcoa.h (libpcoa_hip.so).

There is no CPU fallback: if the HIP library is missing this module raises ImportError, and without a
GPU pcoa_create fails with PCOA_ERR_NO_DEVICE.  Nothing here imports oracle/.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCOA_LIB: another build of the same library (A/B runs of two trees on one box, sanitizer builds); there is no fallback
# either way -- the named file is loaded or the import fails
LIB_PATH = os.environ.get("PCOA_LIB") or os.path.join(_HERE, "libpcoa_hip.so")

PCOA_OK = 0
PCOA_ERR_INVALID_ARG = -1
PCOA_ERR_NO_DEVICE = -2
PCOA_ERR_HIP = -3
PCOA_ERR_OUT_OF_MEMORY = -4
PCOA_ERR_INDEX_RANGE = -5
PCOA_ERR_RCCL = -6
PCOA_ERR_NOT_CONVERGED = -7
PCOA_ERR_STATE = -8

PCOA_FLAG_DEFAULT = 0
PCOA_FLAG_GRAM_F32_MFMA = 0x1
PCOA_FLAG_GRAM_I8_MFMA = 0x2
PCOA_FLAG_GRAM_FP4_MFMA = 0x4
PCOA_FLAG_NO_SIGN_NORM = 0x10
PCOA_FLAG_EIG_HOUSEHOLDER = 0x20
PCOA_FLAG_EIG_LANCZOS = 0x40
PCOA_FLAG_NO_PIPELINE = 0x80
PCOA_FLAG_OPERAND_FP4 = 0x100
PCOA_FLAG_EIG_BAND = 0x200
PCOA_LAYOUT_AUTO = 0
PCOA_LAYOUT_FULL = 1
PCOA_LAYOUT_STRIPS = 2
PCOA_LAYOUT_FREE_FRACTION = 0.9
MATVEC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
PCOA_BED_HOST_ASYNC = 2
PCOA_CALLS_DEVICE_PTR = 1
PCOA_CALLS_HOST_PINNED = 2
PCOA_CALLS_ASYNC = 4


class PcoaTimings(ctypes.Structure):
    _fields_ = [
        ("gram_kernel_seconds", ctypes.c_double),
        ("gram_kernel_launches", ctypes.c_int64),
        ("gram_variants", ctypes.c_int64),
        ("gram_flops", ctypes.c_double),
        ("gram_bytes", ctypes.c_double),
        ("densify_seconds", ctypes.c_double),
        ("synth_seconds", ctypes.c_double),
        ("finalize_seconds", ctypes.c_double),
        ("center_seconds", ctypes.c_double),
        ("tridiag_seconds", ctypes.c_double),
        ("eig_seconds", ctypes.c_double),
        ("backtransform_seconds", ctypes.c_double),
        ("compute_total_seconds", ctypes.c_double),
        ("gram_kernel_kind", ctypes.c_int32),
        ("operand_bits", ctypes.c_int32),
        ("pack_seconds", ctypes.c_double),
        ("pack_launches", ctypes.c_int64),
        ("pack_bytes", ctypes.c_double),
        ("lanczos_seconds", ctypes.c_double),
        ("eig_method", ctypes.c_int32),
        ("lanczos_steps", ctypes.c_int32),
        ("fp4_fallbacks", ctypes.c_int64),
        ("lockstep_launches", ctypes.c_int64),
        ("pipeline_launches", ctypes.c_int64),
        ("pipeline_pre_pass_cus", ctypes.c_int32),
        ("pipeline_contraction_cus", ctypes.c_int32),
        ("evensplit_launches", ctypes.c_int64),
        ("csr_stage_seconds", ctypes.c_double),
        ("csr_wait_seconds", ctypes.c_double),
        ("csr_fast_chunks", ctypes.c_int64),
        ("csr_redo_chunks", ctypes.c_int64),
        ("allreduce_seconds", ctypes.c_double),
        ("allreduce_calls", ctypes.c_int64),
        ("comm_ranks", ctypes.c_int32),
        ("allreduce_int32", ctypes.c_int32),
        ("matvec_form", ctypes.c_int32),
        ("gram_i64_live", ctypes.c_int32),
        ("reduce_int32_calls", ctypes.c_int64),
        ("narrowed_to_int32", ctypes.c_int64),
        ("lanczos_block_steps", ctypes.c_int32),
        ("eig_dense_form", ctypes.c_int32),
        ("operator_products", ctypes.c_int64),
        ("operator_matvec_seconds", ctypes.c_double),
        ("operator_store_bytes", ctypes.c_int64),
        ("subset_seconds", ctypes.c_double),
        ("subset_bytes", ctypes.c_int64),
    ]


class PcoaReducePeersStats(ctypes.Structure):
    """pcoa_reduce_peers_stats: a struct of its own beside pcoa_timings, whose layout and size are held fixed."""
    _fields_ = [
        ("reduce_peers_calls", ctypes.c_int64),
        ("reduce_peers_seconds", ctypes.c_double),
        ("reduce_peers_bytes_in", ctypes.c_int64),
    ]


PCOA_REDUCE_MAX_ENGINES = 16


class PcoaPair(ctypes.Structure):
    """pcoa_pair: one reported pair of pcoa_similar_pairs, i < j, shared = S(i, j); 16 bytes."""
    _fields_ = [
        ("i", ctypes.c_int32),
        ("j", ctypes.c_int32),
        ("shared", ctypes.c_int64),
    ]


class PcoaPairsStats(ctypes.Structure):
    """pcoa_pairs_stats: a struct of its own beside pcoa_timings, like pcoa_reduce_peers_stats."""
    _fields_ = [
        ("pairs_seconds", ctypes.c_double),
        ("pairs_bytes", ctypes.c_int64),
        ("pairs_calls", ctypes.c_int64),
    ]


PCOA_KING_HET = 0
PCOA_KING_MISSING = 1
PCOA_KING_HET_OR_MISSING = 2
PCOA_KING_HOM_A1 = 3
PCOA_KING_HOM_A2 = 4
PCOA_KING_PLANES = 5


class PcoaKingPair(ctypes.Structure):
    """pcoa_king_pair: one reported pair of pcoa_king_pairs, i < j, with the three counts of the rule; 32 bytes."""
    _fields_ = [
        ("i", ctypes.c_int32),
        ("j", ctypes.c_int32),
        ("hethet", ctypes.c_int64),
        ("ibs0", ctypes.c_int64),
        ("het_sum", ctypes.c_int64),
    ]


class PcoaKingStats(ctypes.Structure):
    """pcoa_king_stats: a struct of its own beside pcoa_timings, like pcoa_pairs_stats."""
    _fields_ = [
        ("king_seconds", ctypes.c_double),
        ("king_bytes", ctypes.c_int64),
        ("king_calls", ctypes.c_int64),
    ]


class PcoaLdStats(ctypes.Structure):
    """pcoa_ld_stats: what the LD pruner did, and the HIP-event time of each of its kernels."""
    _fields_ = [
        ("ld_variants", ctypes.c_int64),
        ("ld_kept", ctypes.c_int64),
        ("ld_monomorphic", ctypes.c_int64),
        ("ld_pairs", ctypes.c_int64),
        ("ld_count_seconds", ctypes.c_double),
        ("ld_band_seconds", ctypes.c_double),
        ("ld_resolve_seconds", ctypes.c_double),
        ("ld_compact_seconds", ctypes.c_double),
    ]


class PcoaLoadingsStats(ctypes.Structure):
    """pcoa_loadings_stats: a struct of its own beside pcoa_timings, like pcoa_pairs_stats."""
    _fields_ = [
        ("loadings_variants", ctypes.c_int64),
        ("loadings_bytes", ctypes.c_int64),
        ("loadings_seconds", ctypes.c_double),
    ]


class PcoaGrmBlockStats(ctypes.Structure):
    """pcoa_grm_block_stats: a struct of its own beside pcoa_timings, like pcoa_pairs_stats."""
    _fields_ = [
        ("grm_block_seconds", ctypes.c_double),
        ("grm_block_calls", ctypes.c_int64),
        ("grm_block_flops", ctypes.c_double),
    ]


class PcoaGrmPair(ctypes.Structure):
    """pcoa_grm_pair: one reported pair of pcoa_grm_pairs, i < j, k = K(i, j), n = n(i, j) or M'; 24 bytes."""
    _fields_ = [
        ("i", ctypes.c_int32),
        ("j", ctypes.c_int32),
        ("k", ctypes.c_double),
        ("n", ctypes.c_int64),
    ]


class PcoaGrmPairsStats(ctypes.Structure):
    """pcoa_grm_pairs_stats: a struct of its own beside pcoa_timings, like pcoa_pairs_stats."""
    _fields_ = [
        ("grm_pairs_seconds", ctypes.c_double),
        ("grm_pairs_screen_seconds", ctypes.c_double),
        ("grm_pairs_calls", ctypes.c_int64),
        ("grm_pairs_bands", ctypes.c_int64),
        ("grm_pairs_flops", ctypes.c_double),
        ("grm_pairs_bytes", ctypes.c_int64),
    ]


class PcoaGrmKingStats(ctypes.Structure):
    """pcoa_grm_king_stats: what pcoa_grm_king_block / pcoa_grm_king_pairs did on the engine."""
    _fields_ = [
        ("grm_king_seconds", ctypes.c_double),
        ("grm_king_screen_seconds", ctypes.c_double),
        ("grm_king_calls", ctypes.c_int64),
        ("grm_king_bands", ctypes.c_int64),
        ("grm_king_macs", ctypes.c_double),
        ("grm_king_bytes", ctypes.c_int64),
        ("grm_king_block_calls", ctypes.c_int64),
    ]


class PcoaGrmPcrelateStats(ctypes.Structure):
    """pcoa_grm_pcrelate_stats: what pcoa_grm_pcrelate_fit / _block / _pairs did on the engine."""
    _fields_ = [
        ("grm_pcrelate_fits", ctypes.c_int64),
        ("grm_pcrelate_block_calls", ctypes.c_int64),
        ("grm_pcrelate_pairs_calls", ctypes.c_int64),
        ("grm_pcrelate_bands", ctypes.c_int64),
        ("grm_pcrelate_fit_seconds", ctypes.c_double),
        ("grm_pcrelate_dense_seconds", ctypes.c_double),
        ("grm_pcrelate_screen_seconds", ctypes.c_double),
        ("grm_pcrelate_flops", ctypes.c_double),
        ("grm_pcrelate_bytes", ctypes.c_int64),
        ("grm_pcrelate_n_cov", ctypes.c_int64),
    ]


class PcoaGrmSubsetStats(ctypes.Structure):
    """pcoa_grm_subset_stats: what pcoa_create_grm_subset did with this engine as its source."""
    _fields_ = [
        ("grm_subset_seconds", ctypes.c_double),
        ("grm_subset_calls", ctypes.c_int64),
        ("grm_subset_bytes", ctypes.c_int64),
    ]


class PcoaGrmLsqStats(ctypes.Structure):
    """pcoa_grm_lsq_stats: what pcoa_grm_project_lsq did with the ctx as the panel."""
    _fields_ = [
        ("grm_lsq_calls", ctypes.c_int64),
        ("grm_lsq_pair_vectors", ctypes.c_int64),
        ("grm_lsq_pairs_seconds", ctypes.c_double),
        ("grm_lsq_solve_seconds", ctypes.c_double),
        ("grm_lsq_undetermined", ctypes.c_int64),
    ]


class PcoaGrmQcStats(ctypes.Structure):
    """pcoa_grm_qc_stats: what the QC calls did, and the variants failing each variant test under the current settings."""
    _fields_ = [
        ("grm_qc_hwe_seconds", ctypes.c_double),
        ("grm_qc_hwe_calls", ctypes.c_int64),
        ("grm_qc_sample_counts_seconds", ctypes.c_double),
        ("grm_qc_sample_counts_calls", ctypes.c_int64),
        ("grm_qc_fail_maf", ctypes.c_int64),
        ("grm_qc_fail_missing", ctypes.c_int64),
        ("grm_qc_fail_hwe", ctypes.c_int64),
    ]


class PcoaGrmLdStats(ctypes.Structure):
    """pcoa_grm_ld_stats: what the last pcoa_grm_ld_prune did, and the HIP-event time of its kernels."""
    _fields_ = [
        ("grm_ld_variants", ctypes.c_int64),
        ("grm_ld_candidates", ctypes.c_int64),
        ("grm_ld_kept", ctypes.c_int64),
        ("grm_ld_pairs", ctypes.c_int64),
        ("grm_ld_band_seconds", ctypes.c_double),
        ("grm_ld_resolve_seconds", ctypes.c_double),
        ("grm_ld_scan_seconds", ctypes.c_double),
    ]


PCOA_GRM_DIVISOR_USED = 0
PCOA_GRM_DIVISOR_PAIRWISE = 1
PCOA_GRM_SUBSET_PANEL = 0
PCOA_GRM_SUBSET_STUDY = 1
PCOA_GRM_ROWS_ALL = 0
PCOA_GRM_ROWS_USED = 1
PCOA_LOADINGS_CENTRE = 1
PCOA_LOADINGS_UNIT = 2
PCOA_LD_MAX_WINDOW = 1024
PCOA_LD_ACCUMULATE = 1


class PcoaSynthParams(ctypes.Structure):
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("n_pops", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("pop_offsets", ctypes.POINTER(ctypes.c_int32)),
        ("thresholds", ctypes.POINTER(ctypes.c_uint32)),
    ]


# every symbol include/pcoa.h declares: (name, restype, argtypes)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_SIGNATURES = [
    ("pcoa_version", ctypes.c_char_p, []),
    ("pcoa_create", ctypes.c_int, [ctypes.POINTER(_vp), _i32, _i32, ctypes.c_uint32]),
    ("pcoa_create_strip", ctypes.c_int, [ctypes.POINTER(_vp), _i32, _i32, _i32, _i32, ctypes.c_uint32]),
    ("pcoa_create_operator", ctypes.c_int, [ctypes.POINTER(_vp), _i32, _i32, ctypes.c_uint32]),
    ("pcoa_create_subset", ctypes.c_int, [ctypes.POINTER(_vp), _vp, _vp, _i32]),
    ("pcoa_similar_pairs", ctypes.c_int, [_vp, ctypes.c_double, _vp, _i64, ctypes.POINTER(_i64), _vp]),
    ("pcoa_get_pairs_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaPairsStats), ctypes.c_size_t]),
    ("pcoa_set_similarity", ctypes.c_int, [_vp, _i32]),
    ("pcoa_get_similarity", ctypes.c_int, [_vp, ctypes.POINTER(_i32)]),
    ("pcoa_set_call_companion", ctypes.c_int, [_vp, _vp, _i64]),
    ("pcoa_get_call_companion", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    ("pcoa_accumulate_plink_bed_calls", ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int]),
    ("pcoa_accumulate_plink_bed_king", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int]),
    ("pcoa_king_pairs", ctypes.c_int, [_vp, ctypes.c_double, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _vp]),
    ("pcoa_get_king_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaKingStats), ctypes.c_size_t]),
    ("pcoa_loadings_begin", ctypes.c_int, [_vp, _i32, _vp, _vp, ctypes.c_uint32]),
    ("pcoa_loadings_bits", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int, _vp, ctypes.c_int]),
    ("pcoa_loadings_plink_bed", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int]),
    ("pcoa_loadings_operator", ctypes.c_int, [_vp, _i64, _i64, _vp, ctypes.c_int]),
    ("pcoa_loadings_end", ctypes.c_int, [_vp]),
    ("pcoa_get_loadings_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaLoadingsStats), ctypes.c_size_t]),
    ("pcoa_ld_begin", ctypes.c_int, [_vp, _i32, ctypes.c_double, ctypes.c_uint32]),
    ("pcoa_ld_bits", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int, _vp, ctypes.POINTER(_i64)]),
    ("pcoa_ld_plink_bed", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_i64)]),
    ("pcoa_ld_break", ctypes.c_int, [_vp]),
    ("pcoa_ld_end", ctypes.c_int, [_vp]),
    ("pcoa_get_ld_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaLdStats), ctypes.c_size_t]),
    ("pcoa_operator_info", ctypes.c_int, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("pcoa_operator_row_sums", ctypes.c_int, [_vp, _vp]),
    ("pcoa_operator_matvec_device", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int]),
    ("pcoa_create_grm", ctypes.c_int, [ctypes.POINTER(_vp), _i32, _i32, ctypes.c_uint32]),
    ("pcoa_grm_info", ctypes.c_int, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("pcoa_grm_set_min_maf", ctypes.c_int, [_vp, ctypes.c_double]),
    ("pcoa_grm_counts", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_grm_matvec_device", ctypes.c_int, [_vp, _vp, _vp]),
    ("pcoa_create_grm_study", ctypes.c_int, [ctypes.POINTER(_vp), _i32, _i32, ctypes.c_uint32]),
    ("pcoa_grm_weights", ctypes.c_int, [_vp, _i32, _vp, _vp, _i32, _i64, _i64, _vp]),
    ("pcoa_grm_project", ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    ("pcoa_grm_project_lsq", ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("pcoa_get_grm_lsq_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmLsqStats), ctypes.c_size_t]),
    ("pcoa_grm_block", ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, ctypes.c_int]),
    ("pcoa_get_grm_block_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmBlockStats), ctypes.c_size_t]),
    ("pcoa_grm_pairs", ctypes.c_int, [_vp, ctypes.c_double, _i32, _i32, _vp, _i64, ctypes.POINTER(_i64), _vp]),
    ("pcoa_get_grm_pairs_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmPairsStats), ctypes.c_size_t]),
    ("pcoa_grm_king_block", ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, ctypes.c_int]),
    ("pcoa_grm_king_pairs", ctypes.c_int, [_vp, _i32, ctypes.c_double, _i32, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _vp]),
    ("pcoa_get_grm_king_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmKingStats), ctypes.c_size_t]),
    ("pcoa_pcrelate_hat", ctypes.c_int, [_i32, _i32, _vp, _vp]),
    ("pcoa_grm_pcrelate_fit", ctypes.c_int, [_vp, _i32, _vp, _vp]),
    ("pcoa_grm_pcrelate_beta", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_grm_pcrelate_isaf", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_grm_pcrelate_block", ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, ctypes.c_double, _vp, _vp, ctypes.c_int]),
    ("pcoa_grm_pcrelate_pairs", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, _i32, _vp, _i64, ctypes.POINTER(_i64), _vp]),
    ("pcoa_get_grm_pcrelate_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmPcrelateStats), ctypes.c_size_t]),
    ("pcoa_grm_ld_prune", ctypes.c_int, [_vp, _i32, ctypes.c_double, _vp, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("pcoa_grm_ld_mask", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_grm_ld_clear", ctypes.c_int, [_vp]),
    ("pcoa_get_grm_ld_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmLdStats), ctypes.c_size_t]),
    ("pcoa_create_grm_subset", ctypes.c_int, [ctypes.POINTER(_vp), _vp, _vp, _i32, _i32]),
    ("pcoa_grm_rows", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_get_grm_subset_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmSubsetStats), ctypes.c_size_t]),
    ("pcoa_grm_set_variant_filters", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double]),
    ("pcoa_grm_get_variant_filters", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    ("pcoa_grm_hwe", ctypes.c_int, [_vp, _i64, _i64, _vp]),
    ("pcoa_grm_sample_counts", ctypes.c_int, [_vp, _i32, _vp]),
    ("pcoa_get_grm_qc_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaGrmQcStats), ctypes.c_size_t]),
    ("pcoa_strip_info", ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    ("pcoa_strip_col_sums", ctypes.c_int, [_vp, _vp]),
    ("pcoa_strip_matvec", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    ("pcoa_strip_set_centering", ctypes.c_int, [_vp, _vp, ctypes.c_double]),
    ("pcoa_strip_matvec_device", ctypes.c_int, [_vp, _vp, _vp]),
    ("pcoa_plan_layout", ctypes.c_int, [_i32, _i32, _vp, _i32, ctypes.POINTER(_i32), _vp, _vp]),
    ("pcoa_device_memory", ctypes.c_int, [_i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("pcoa_compute_strips", ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, ctypes.POINTER(_i32)]),
    ("pcoa_project", ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    ("pcoa_destroy", None, [_vp]),
    ("pcoa_last_error", ctypes.c_char_p, [_vp]),
    ("pcoa_reset", ctypes.c_int, [_vp]),
    ("pcoa_n_samples", ctypes.c_int, [_vp]),
    ("pcoa_set_stream", ctypes.c_int, [_vp, _vp]),
    ("pcoa_sync", ctypes.c_int, [_vp]),
    ("pcoa_reserve", ctypes.c_int, [_vp, _i64, _i32]),
    ("pcoa_comm_runtime", ctypes.c_int, [ctypes.c_char_p, _i32, ctypes.POINTER(_i32)]),
    ("pcoa_debug_alloc", ctypes.c_int, [_i32, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    ("pcoa_debug_free", ctypes.c_int, [_vp]),
    ("pcoa_debug_reduce_chunk", ctypes.c_int, [_i32, _i32, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("pcoa_debug_guard_mode", ctypes.c_int, []),
    ("pcoa_accumulate_calls", ctypes.c_int, [_vp, _vp, _vp, _i64]),
    ("pcoa_gram_reduce_from", ctypes.c_int, [_vp, _vp]),
    ("pcoa_gram_reduce_peers", ctypes.c_int, [_vp, _i32, _i32]),
    ("pcoa_get_reduce_peers_stats", ctypes.c_int, [_vp, ctypes.POINTER(PcoaReducePeersStats), ctypes.c_size_t]),
    ("pcoa_lanczos_with_matvec", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32)]),
    ("pcoa_debug_centred_matvec", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int]),
    ("pcoa_host_alloc_pinned", ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    ("pcoa_host_free_pinned", ctypes.c_int, [_vp]),
    ("pcoa_accumulate_plink_bed", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int, ctypes.c_int]),
    ("pcoa_accumulate_calls_ex", ctypes.c_int, [_vp, _vp, _vp, _i64, ctypes.c_uint32]),
    ("pcoa_accumulate_dense_f32", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int]),
    ("pcoa_accumulate_dense_u8", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int]),
    ("pcoa_accumulate_bits", ctypes.c_int, [_vp, _vp, _i64, _i64, ctypes.c_int]),
    ("pcoa_accumulate_synthetic", ctypes.c_int, [_vp, ctypes.POINTER(PcoaSynthParams), _i64, _i64]),
    ("pcoa_synth_fill_f32", ctypes.c_int, [_vp, ctypes.POINTER(PcoaSynthParams), _i64, _i64, _vp, _i64]),
    ("pcoa_gram_finalize", ctypes.c_int, [_vp]),
    ("pcoa_gram_allreduce_rccl", ctypes.c_int, [_vp, _vp]),
    ("pcoa_comm_unique_id", ctypes.c_int, [_vp]),
    ("pcoa_comm_init", ctypes.c_int, [_vp, _vp, _i32, _i32, ctypes.POINTER(_vp)]),
    ("pcoa_comm_destroy", ctypes.c_int, [_vp]),
    ("pcoa_comm_count", ctypes.c_int, [_vp, ctypes.POINTER(_i32)]),
    ("pcoa_gram_export_device_i64", ctypes.c_int, [_vp, _vp]),
    ("pcoa_gram_import_device_i64", ctypes.c_int, [_vp, _vp]),
    ("pcoa_gram_read_i64", ctypes.c_int, [_vp, _vp]),
    ("pcoa_gram_read_block_i64", ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp]),
    ("pcoa_gram_load_i64", ctypes.c_int, [_vp, _vp]),
    ("pcoa_center_read_f64", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(_i32), ctypes.POINTER(ctypes.c_double)]),
    ("pcoa_compute", ctypes.c_int, [_vp, _i32, _vp, _vp, ctypes.POINTER(_i32)]),
    ("pcoa_get_timings", ctypes.c_int, [_vp, ctypes.POINTER(PcoaTimings)]),
    ("pcoa_get_timings_sized", ctypes.c_int, [_vp, ctypes.POINTER(PcoaTimings), ctypes.c_size_t]),
    ("pcoa_reset_timings", ctypes.c_int, [_vp]),
    ("pcoa_device_info", ctypes.c_int, [_vp, ctypes.c_char_p, _i32, ctypes.POINTER(_i32)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None


def source_hash():
    """sha256 (first 16 hex digits) over the kernel sources the library is built from (csrc/* and include/pcoa.h).
    A measurement file made from one tree (profiles/gram_pmc_live.json) names the tree by this hash; .git does not
    travel to the GPU box and the commit that adds such a file moves HEAD, so a commit id cannot be used for it."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".inl", ".h"))]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "pcoa.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """Loads libpcoa_hip.so and binds every entry point; raises ImportError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C spark-examples_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  If libpcoa_hip.so pulls in
    # /opt/rocm's copy first and torch is imported later, two runtimes tear down at exit ("double free or
    # corruption").  Importing torch first makes the loader resolve our DT_NEEDED entry to the runtime
    # that is already mapped.  (Plumbing only; skipped when torch is not installed.)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, restype, argtypes in _SIGNATURES:
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib
