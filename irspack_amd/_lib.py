"""ctypes loader for ``libirspack_amd.so`` (the C ABI of include/irspack_amd.h).

Loading fails loudly when the shared library has not been built; compute calls
fail loudly (``RuntimeError``) when no HIP device is visible.  There is no
fallback implementation.
"""

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IRSPACK_AMD_LIB selects another build of the same ABI (kernel tuning experiments)
LIB_PATH = os.environ.get("IRSPACK_AMD_LIB") or os.path.join(_HERE, "libirspack_amd.so")


class ModelConfigStruct(C.Structure):
    _fields_ = [
        ("K", C.c_uint64),
        ("alpha0", C.c_float),
        ("reg", C.c_float),
        ("nu", C.c_float),
        ("init_stdev", C.c_float),
        ("random_seed", C.c_int32),
        ("loss_type", C.c_int32),
        ("lambda_user_feature", C.c_float),
        ("lambda_item_feature", C.c_float),
        ("feature_warmup_epochs", C.c_uint64),
    ]


class SolverConfigStruct(C.Structure):
    _fields_ = [
        ("n_threads", C.c_uint64),
        ("solver_type", C.c_int32),
        ("max_cg_steps", C.c_uint64),
        ("ialspp_subspace_dimension", C.c_uint64),
        ("ialspp_iteration", C.c_uint64),
    ]


class ShardStruct(C.Structure):
    _fields_ = [
        ("user_begin", C.c_int64),
        ("user_end", C.c_int64),
        ("item_begin", C.c_int64),
        ("item_end", C.c_int64),
    ]


class MetricsStruct(C.Structure):
    _fields_ = [
        ("valid_user", C.c_uint64),
        ("total_user", C.c_uint64),
        ("hit", C.c_double),
        ("recall", C.c_double),
        ("ndcg", C.c_double),
        ("precision", C.c_double),
        ("map", C.c_double),
    ]


class EvalStatsStruct(C.Structure):  # irs_eval_stats
    _fields_ = [
        ("path", C.c_int32),
        ("hard_rows", C.c_int32),
        ("tiles_total", C.c_int64),
        ("tiles_scored", C.c_int64),
        ("sample_items", C.c_int64),
        ("call_ms", C.c_double),
        ("device_span_ms", C.c_double),
    ]


class CeilingsStruct(C.Structure):  # irs_ceilings
    _fields_ = [
        ("copy_gbs", C.c_double),
        ("triad_gbs", C.c_double),
        ("mfma_f32_tflops", C.c_double),
        ("lds_atomic_u32_gops", C.c_double),
        ("clock_mhz", C.c_double),
        ("n_cu", C.c_int32),
        ("gather256_gbs", C.c_double),
        ("gather512_gbs", C.c_double),
    ]


class DenseSlimStatsStruct(C.Structure):  # irs_dense_slim_stats
    _fields_ = [
        ("gram_ms", C.c_double),
        ("factor_ms", C.c_double),
        ("invert_ms", C.c_double),
        ("finalize_ms", C.c_double),
        ("d2h_ms", C.c_double),
        ("n_pad", C.c_int64),
    ]


class TruncSvdStatsStruct(C.Structure):  # irs_truncsvd_stats_t
    _fields_ = [
        ("setup_ms", C.c_double),
        ("spmm_ms", C.c_double),
        ("gram_ms", C.c_double),
        ("chol_ms", C.c_double),
        ("apply_ms", C.c_double),
        ("d2h_ms", C.c_double),
        ("host_ms", C.c_double),
        ("n_spmm", C.c_int64),
        ("l_pad", C.c_int64),
    ]


class NmfStatsStruct(C.Structure):  # irs_nmf_stats_t
    _fields_ = [
        ("setup_ms", C.c_double),
        ("spmm_ms", C.c_double),
        ("gram_ms", C.c_double),
        ("sweep_ms", C.c_double),
        ("d2h_ms", C.c_double),
    ]


class BprStatsStruct(C.Structure):  # irs_bpr_stats_t
    _fields_ = [
        ("n_positives", C.c_int64),
        ("n_skipped_full_rows", C.c_int64),
        ("n_skipped_positives", C.c_int64),
        ("batches_per_epoch", C.c_int64),
        ("lanes_per_triple", C.c_int32),
        ("scale_log2", C.c_int32),
        ("epoch_ms", C.c_double),
        ("sample_ms", C.c_double),
        ("grad_ms", C.c_double),
        ("apply_ms", C.c_double),
    ]


class BprWarpStatsStruct(C.Structure):  # irs_bpr_warp_stats_t
    _fields_ = [
        ("max_sampled", C.c_int32),
        ("scale_log2", C.c_int32),
        ("in_flight", C.c_int32),
        ("reserved", C.c_int32),
        ("epoch_positions", C.c_int64),
        ("epoch_updates", C.c_int64),
        ("epoch_tries", C.c_int64),
        ("call_positions", C.c_int64),
        ("call_updates", C.c_int64),
        ("call_tries", C.c_int64),
        ("epoch_ms", C.c_double),
        ("search_ms", C.c_double),
        ("apply_ms", C.c_double),
    ]


class MultVaeStatsStruct(C.Structure):  # irs_multvae_stats_t
    _fields_ = [
        ("n_updates", C.c_int64),
        ("epoch", C.c_int64),
        ("batches_per_epoch", C.c_int64),
        ("dh2_slab", C.c_int32),
        ("dw4_slab", C.c_int32),
        ("scale_log2", C.c_int32),
        ("reserved", C.c_int32),
        ("klc_next", C.c_double),
        ("klc_last", C.c_double),
        ("nll_last", C.c_double),
        ("kl_last", C.c_double),
        ("epoch_ms", C.c_double),
        ("encode_ms", C.c_double),
        ("dense_ms", C.c_double),
        ("logit_ms", C.c_double),
        ("softmax_ms", C.c_double),
        ("dw4_ms", C.c_double),
        ("dh2_ms", C.c_double),
        ("dw1_ms", C.c_double),
        ("adam_ms", C.c_double),
    ]


class SplitStatsStruct(C.Structure):  # irs_split_stats
    _fields_ = [
        ("upload_ms", C.c_double),
        ("select_ms", C.c_double),
        ("scan_ms", C.c_double),
        ("scatter_ms", C.c_double),
        ("d2h_ms", C.c_double),
        ("rows_empty", C.c_int64),
        ("rows_wave", C.c_int64),
        ("rows_lds", C.c_int64),
        ("rows_stream", C.c_int64),
    ]


SPLIT_BY_RATIO, SPLIT_BY_FIXED_N = 0, 1  # IRS_SPLIT_BY_* of include/irspack_amd.h

ABI_VERSION = 4  # IRS_ABI_VERSION of include/irspack_amd.h
# the metrics of irs_serve_neighbors
NEIGHBOR_WEIGHT, NEIGHBOR_COSINE, NEIGHBOR_DOT = 0, 1, 2
# IRS_EXCHANGE_* of include/irspack_amd.h: how irs_ials_sharded_step moves the solved rows
EXCHANGE_MODES = {"auto": 0, "broadcast": 1, "mesh": 2, "peer": 3}
COMM_HANDLE_BYTES = 256

# every symbol include/irspack_amd.h declares
EXPORTED_SYMBOLS = [
    "irs_last_error",
    "irs_abi_version",
    "irs_device_count",
    "irs_ials_create",
    "irs_ials_create_from_factors",
    "irs_ials_destroy",
    "irs_ials_step",
    "irs_ials_get_factor",
    "irs_ials_set_factor",
    "irs_ials_user_scores",
    "irs_ials_transform",
    "irs_ials_transform_with_prior",
    "irs_ials_set_prior",
    "irs_ials_set_features",
    "irs_ials_apply_feature_prior",
    "irs_ials_feature_rhs",
    "irs_ials_feature_step",
    "irs_ials_get_feature_weight",
    "irs_ials_set_feature_weight",
    "irs_ials_compute_loss",
    "irs_ials_set_stream",
    "irs_ials_device_buffer",
    "irs_ials_copy_rows_async",
    "irs_ials_partial_gramian_async",
    "irs_ials_finish_gramian_async",
    "irs_ials_gramian_async",
    "irs_ials_half_step_async",
    "irs_ials_synchronize",
    "irs_comm_unique_id",
    "irs_comm_create",
    "irs_comm_create_local",
    "irs_comm_destroy",
    "irs_comm_export",
    "irs_comm_attach",
    "irs_comm_set_exchange",
    "irs_comm_get_exchange",
    "irs_ials_sharded_step",
    "irs_ials_last_eigenbasis",
    "irs_ials_eigen_debug",
    "irs_ials_profile",
    "irs_ials_profile_read",
    "irs_knn_create",
    "irs_knn_weight",
    "irs_knn_destroy",
    "irs_knn_compute",
    "irs_knn_fetch",
    "irs_knn_fetch_csc",
    "irs_knn_last_stats",
    "irs_knn_last_walked",
    "irs_remove_diagonal",
    "irs_retrieve_recommend",
    "irs_slim_fit",
    "irs_slim_nnz",
    "irs_slim_fetch",
    "irs_slim_last_stats",
    "irs_slim_last_launch",
    "irs_slim_destroy",
    "irs_split_rowwise",
    "irs_split_nnz",
    "irs_split_fetch",
    "irs_split_last_stats",
    "irs_split_destroy",
    "irs_dense_slim_fit",
    "irs_truncsvd_create",
    "irs_truncsvd_range",
    "irs_truncsvd_apply",
    "irs_truncsvd_project",
    "irs_truncsvd_finish",
    "irs_truncsvd_stats",
    "irs_truncsvd_destroy",
    "irs_truncsvd_transform",
    "irs_nmf_fit",
    "irs_bpr_create",
    "irs_bpr_run_epochs",
    "irs_bpr_sample",
    "irs_bpr_step_triples",
    "irs_bpr_get_state",
    "irs_bpr_set_state",
    "irs_bpr_stats",
    "irs_bpr_destroy",
    "irs_bpr_create_warp",
    "irs_bpr_warp_candidates",
    "irs_bpr_warp_search",
    "irs_bpr_warp_step",
    "irs_bpr_warp_stats",
    "irs_multvae_create",
    "irs_multvae_run_epochs",
    "irs_multvae_order",
    "irs_multvae_noise",
    "irs_multvae_step_batch",
    "irs_multvae_gradients",
    "irs_multvae_get_state",
    "irs_multvae_set_state",
    "irs_multvae_encode",
    "irs_multvae_score",
    "irs_multvae_stats",
    "irs_multvae_destroy",
    "irs_eval_create",
    "irs_eval_destroy",
    "irs_eval_get_metrics",
    "irs_eval_get_metrics_masked",
    "irs_eval_get_metrics_similarity",
    "irs_eval_get_metrics_dense_similarity",
    "irs_eval_get_metrics_factors",
    "irs_eval_get_metrics_similarity_scored",
    "irs_eval_get_metrics_dense_similarity_scored",
    "irs_eval_get_metrics_factors_scored",
    "irs_eval_last_phases",
    "irs_eval_get_metrics_ials",
    "irs_eval_cache_mask",
    "irs_eval_last_stats",
    "irs_fingerprint",
    "irs_serve_create_similarity",
    "irs_serve_create_dense_similarity",
    "irs_serve_create_factors",
    "irs_serve_destroy",
    "irs_serve_recommend_profiles",
    "irs_serve_recommend_factors",
    "irs_serve_neighbors",
    "irs_serve_last_phases",
    "irs_measure_ceilings",
]

# argument types of the feature-aware step, its weight accessors and the SLIM calls (irs_status return)
ARGTYPES = {
    "irs_ials_feature_step": [C.c_void_p, C.c_void_p],
    "irs_ials_get_feature_weight": [C.c_void_p, C.c_int32, C.POINTER(C.c_float)],
    "irs_ials_set_feature_weight": [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_int64, C.c_int64],
    "irs_slim_fit": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                     C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_int32,
                     C.POINTER(C.c_void_p)],
    "irs_slim_nnz": [C.c_void_p, C.POINTER(C.c_int64)],
    "irs_slim_fetch": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)],
    "irs_slim_last_stats": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                            C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "irs_slim_last_launch": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "irs_slim_destroy": [C.c_void_p],
    "irs_split_rowwise": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                          C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)],
    "irs_split_nnz": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "irs_split_fetch": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64),
                        C.POINTER(C.c_int32), C.c_void_p],
    "irs_split_last_stats": [C.c_void_p, C.c_void_p],
    "irs_split_destroy": [C.c_void_p],
    "irs_dense_slim_fit": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                           C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_float), C.c_void_p],
    "irs_truncsvd_create": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                            C.c_int32, C.POINTER(C.c_void_p)],
    "irs_truncsvd_range": [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_float)],
    "irs_truncsvd_apply": [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float)],
    "irs_truncsvd_project": [C.c_void_p, C.POINTER(C.c_float)],
    "irs_truncsvd_finish": [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "irs_truncsvd_stats": [C.c_void_p, C.c_void_p],
    "irs_truncsvd_destroy": [C.c_void_p],
    "irs_truncsvd_transform": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                               C.c_int64, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float)],
    "irs_nmf_fit": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int64,
                    C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_double,
                    C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p],
    "irs_bpr_create": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                       C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_uint64, C.POINTER(C.c_float),
                       C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_void_p)],
    "irs_bpr_run_epochs": [C.c_void_p, C.c_int64],
    "irs_bpr_sample": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                       C.POINTER(C.c_int32)],
    "irs_bpr_step_triples": [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "irs_bpr_get_state": [C.c_void_p] + [C.POINTER(C.c_float)] * 6 + [C.POINTER(C.c_int64)],
    "irs_bpr_set_state": [C.c_void_p] + [C.POINTER(C.c_float)] * 6 + [C.c_int64],
    "irs_bpr_stats": [C.c_void_p, C.c_void_p],
    "irs_bpr_destroy": [C.c_void_p],
    "irs_bpr_create_warp": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                            C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_uint64, C.POINTER(C.c_float),
                            C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)],
    "irs_bpr_warp_candidates": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "irs_bpr_warp_search": [C.c_void_p, C.c_int64] + [C.POINTER(C.c_int32)] * 5,
    "irs_bpr_warp_step": [C.c_void_p, C.c_int64] + [C.POINTER(C.c_int32)] * 3,
    "irs_bpr_warp_stats": [C.c_void_p, C.c_void_p],
    "irs_multvae_create": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                           C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_int64, C.c_int64,
                           C.c_float, C.c_uint64, C.POINTER(C.POINTER(C.c_float)), C.c_int32, C.POINTER(C.c_void_p)],
    "irs_multvae_run_epochs": [C.c_void_p, C.c_int64],
    "irs_multvae_order": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32)],
    "irs_multvae_noise": [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                          C.POINTER(C.c_float)],
    "irs_multvae_step_batch": [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float),
                               C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "irs_multvae_gradients": [C.c_void_p, C.POINTER(C.POINTER(C.c_float))],
    "irs_multvae_get_state": [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "irs_multvae_set_state": [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.c_int64, C.c_int64],
    "irs_multvae_encode": [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                           C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "irs_multvae_score": [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                          C.POINTER(C.c_float)],
    "irs_multvae_stats": [C.c_void_p, C.c_void_p],
    "irs_multvae_destroy": [C.c_void_p],
    "irs_eval_get_metrics_dense_similarity": [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
        C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
        C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)],
    "irs_eval_get_metrics_factors": [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
        C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int32,
        C.c_void_p, C.POINTER(C.c_int64)],
    "irs_eval_get_metrics_similarity_scored": [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
        C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64,
        C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int32,
        C.c_void_p, C.POINTER(C.c_int64)],
    "irs_eval_get_metrics_dense_similarity_scored": [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
        C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
        C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)],
    "irs_eval_get_metrics_factors_scored": [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64,
        C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int32,
        C.c_void_p, C.POINTER(C.c_int64)],
    "irs_eval_last_phases": [C.c_void_p, C.POINTER(C.c_double)],
    "irs_serve_create_similarity": [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_void_p)],
    "irs_serve_create_dense_similarity": [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                          C.POINTER(C.c_void_p)],
    "irs_serve_create_factors": [C.c_int64, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_void_p)],
    "irs_serve_destroy": [C.c_void_p],
    "irs_serve_recommend_profiles": [
        C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double),
        C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
        C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32)],
    "irs_serve_recommend_factors": [
        C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int64,
        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float),
        C.POINTER(C.c_int32)],
    "irs_serve_neighbors": [
        C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
        C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float),
        C.POINTER(C.c_int32)],
    "irs_serve_last_phases": [C.c_void_p, C.POINTER(C.c_double)],
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C irspack_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "irspack_amd has no fallback implementation."
            )
        _lib = C.CDLL(LIB_PATH)
        _lib.irs_last_error.restype = C.c_char_p
        _lib.irs_abi_version.restype = C.c_int32
        _lib.irs_device_count.restype = C.c_int32
        for name, args in ARGTYPES.items():
            getattr(_lib, name).argtypes = args
            getattr(_lib, name).restype = C.c_int32
        if _lib.irs_abi_version() != ABI_VERSION:
            found = _lib.irs_abi_version()
            _lib = None
            raise RuntimeError(
                f"{LIB_PATH} has struct layout version {found}, this package was written against "
                f"{ABI_VERSION} (include/irspack_amd.h): rebuild it with `make -C irspack_amd/csrc`.")
    return _lib


def check(status: int) -> None:
    """Map an irs_status to the exception the reference raises."""
    if status == 0:
        return
    msg = lib().irs_last_error().decode("utf-8", "replace")
    if status == 1:
        raise ValueError(msg)
    raise RuntimeError(msg)


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def ptr_array(arrays, ctype):
    """a C array of pointers to the arrays (``None`` stays NULL); the arrays must outlive the call"""
    out = (C.POINTER(ctype) * len(arrays))()
    for q, a in enumerate(arrays):
        if a is not None:
            out[q] = ptr(a, ctype)
    return out


def device_count() -> int:
    return int(lib().irs_device_count())


def measure_ceilings(device: Optional[int] = None) -> dict:
    """Measured device ceilings (irs_measure_ceilings) as a dict."""
    st = CeilingsStruct()
    check(lib().irs_measure_ceilings(C.c_int32(default_device() if device is None else device),
                                     C.byref(st)))
    return {name: getattr(st, name) for name, _ in CeilingsStruct._fields_}


def default_device() -> int:
    """LOCAL_RANK when launched one process per GPU, else IRSPACK_AMD_DEVICE or 0."""
    for key in ("IRSPACK_AMD_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(key)
        if v is not None:
            try:
                return int(v)
            except ValueError:
                pass
    return 0


LAYOUT_CSR, LAYOUT_CSC = 0, 1  # IRS_LAYOUT_* of include/irspack_amd.h
WEIGHT_NONE, WEIGHT_TF_IDF, WEIGHT_BM25 = 0, 1, 2  # IRS_WEIGHT_*


class KnnInputStruct(C.Structure):  # irs_knn_input
    _fields_ = [
        ("layout", C.c_int32),
        ("weighting", C.c_int32),
        ("smooth", C.c_int32),
        ("reserved", C.c_int32),
        ("k1", C.c_double),
        ("b", C.c_double),
    ]


def sparse_arrays(X, dtype):
    """scipy sparse -> (matrix, layout, indptr int64, indices int32, data dtype) WITHOUT changing the
    layout: a CSC matrix (what ``X.T`` of a CSR is - a view of the same arrays) is handed to the library
    as it is (IRS_LAYOUT_CSC), like nanobind's Eigen caster takes either; anything else becomes CSR.
    Indices sorted (a transposed view inherits the flag of its base)."""
    import scipy.sparse as sps

    if sps.isspmatrix_csc(X):
        layout = LAYOUT_CSC
    else:
        layout = LAYOUT_CSR
        if not sps.isspmatrix_csr(X):
            X = sps.csr_matrix(X)
    if not X.has_sorted_indices:
        X = X.sorted_indices()
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    data = np.ascontiguousarray(X.data, dtype=dtype)
    return X, layout, indptr, indices, data


def csr_arrays(X, dtype):
    """scipy sparse -> (csr, indptr int64, indices int32, data dtype) with sorted indices."""
    import scipy.sparse as sps

    # (an existing CSR matrix is used as it is: scipy caches its "sorted" flag on the object, a
    # fresh wrapper would rescan the indices - 4 ms for 20 M entries - on every call)
    if not sps.isspmatrix_csr(X):
        X = sps.csr_matrix(X)
    if not X.has_sorted_indices:
        X = X.sorted_indices()
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    data = np.ascontiguousarray(X.data, dtype=dtype)
    return X, indptr, indices, data
