"""ctypes binding of ``libcss_hip.so`` (the C ABI declared in ``include/css_hip.h``).

There is deliberately no CPU fallback here: if the shared library is missing,
or no HIP device is present when a compute entry point is called, the caller
gets a ``RuntimeError`` carrying ``css_last_error()``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p
from pathlib import Path

_PKG = Path(__file__).resolve().parent
# CSS_HIP_LIB: development aid -- another build of the same library (A/B timing of two source states in one
# GPU session, tools/build_variant.sh); the product always loads the in-tree file.
LIB_PATH = Path(os.environ["CSS_HIP_LIB"]) if os.environ.get("CSS_HIP_LIB") else _PKG / "libcss_hip.so"

CSS_OK = 0
CSS_ERR_INVALID = -1
CSS_ERR_NO_DEVICE = -2
CSS_ERR_HIP = -3
CSS_ERR_OOM = -4
CSS_ERR_STATE = -5
METRIC_IP = 0
METRIC_L2 = 1
MAX_K = 2048   # include/css_hip.h CSS_MAX_K
MAX_GROUP_K = 128   # css_index_search_grouped: the kernels' list size
MAX_DIVERSE_FETCH = 128   # css_index_search_diverse: the largest candidate pool (the same list size)
MAX_PRIOR_K = 128   # css_index_search_prior: the same list size
MAX_HYBRID_K = 128   # css_index_search_hybrid: the same list size
MAX_QUERY_TERMS = 32   # include/css_hip.h CSS_MAX_QUERY_TERMS
TERM_SPACE = 1 << 24   # include/css_hip.h CSS_TERM_SPACE
MAX_SPARSE_QUERY_TERMS = 64   # include/css_hip.h CSS_MAX_SPARSE_QUERY_TERMS
MAX_SPARSE_ROW_ENTRIES = 65536   # include/css_hip.h CSS_MAX_SPARSE_ROW_ENTRIES
MAX_SPARSE_WEIGHT = 65536.0   # include/css_hip.h CSS_MAX_SPARSE_WEIGHT
SPARSE_TOPK_MIN_SLICE = 4096   # csrc/css_sparse.h kSparseTopkMinSlice: rows per block of the column top-k at least ...
SPARSE_TOPK_MAX_PARTS = 32   # ... kSparseTopkMaxParts: and at most this many blocks
MAX_TOKEN_DIM = 128   # include/css_hip.h CSS_MAX_TOKEN_DIM
MAX_ROW_TOKEN_VECTORS = 512   # include/css_hip.h CSS_MAX_ROW_TOKEN_VECTORS
MAX_QUERY_TOKENS = 64   # include/css_hip.h CSS_MAX_QUERY_TOKENS
MAX_MAXSIM_ROWS = 65536   # include/css_hip.h CSS_MAX_MAXSIM_ROWS
MAX_MAXSIM_QUERIES = 1024   # include/css_hip.h CSS_MAX_MAXSIM_QUERIES
MAXSIM_BATCH_GROUP = 8   # include/css_hip.h CSS_MAXSIM_BATCH_GROUP
MAX_SIG_TERMS = 256   # include/css_hip.h CSS_MAX_SIG_TERMS
MAX_FACET_BUCKETS = 1 << 20   # include/css_hip.h CSS_MAX_FACET_BUCKETS
MAX_EXAMPLES = 16   # include/css_hip.h CSS_MAX_EXAMPLES
MAX_EXAMPLES_K = 128   # css_index_search_examples: the same list size
MAX_CENTROIDS = 4096   # include/css_hip.h CSS_MAX_CENTROIDS
MAX_TRANSFORM_ROWS = 256   # include/css_hip.h CSS_MAX_TRANSFORM_ROWS
MAX_ATTRS = 16   # include/css_hip.h CSS_MAX_ATTRS
MAX_CLAUSES = 16   # include/css_hip.h CSS_MAX_CLAUSES
MAX_TABLE_BITS = 1 << 27   # include/css_hip.h CSS_MAX_TABLE_BITS
ATTR_I32, ATTR_F32 = 0, 1   # include/css_hip.h CSS_ATTR_*
WHERE_OPS = ("==", "!=", "<", "<=", ">", ">=", "in", "not in")   # include/css_hip.h CSS_WHERE_*: the index is the code
WHERE_TILE_ROWS = 1024   # csrc/css_where.h kWhereTileRows: rows of one tile of k_where
WHERE_LDS_WORDS = 8192   # csrc/css_where.h kWhereLdsWords: table words of a call that still go to LDS


class CssError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libcss_hip error {code}: {message}")
        self.code = code


class DevInfo(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 128),
        ("gcn_arch", ctypes.c_char * 64),
        ("compute_units", c_int),
        ("wavefront_size", c_int),
        ("hbm_total_bytes", c_int64),
        ("hbm_free_bytes", c_int64),
        ("lds_bytes_per_cu", c_int),
        ("clock_mhz", c_int),
    ]


class Clause(ctypes.Structure):
    """include/css_hip.h css_clause."""
    _fields_ = [
        ("slot", ctypes.c_int32),
        ("op", ctypes.c_int32),
        ("value", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("table_off", c_int64),
        ("table_bits", c_int64),
    ]


class EncoderCfg(ctypes.Structure):
    _fields_ = [
        ("num_layers", c_int),
        ("hidden", c_int),
        ("heads", c_int),
        ("ffn", c_int),
        ("vocab", c_int),
        ("max_pos", c_int),
        ("rel_buckets", c_int),
        ("pad_id", c_int),
        ("max_seq_len", c_int),
        ("ln_eps", c_float),
        ("compute", c_int),
        ("arch", c_int),      # 0 = MPNet, 1 = BERT
        ("pooling", c_int),   # 0 = mean, 1 = CLS
    ]


class Tensor(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", POINTER(c_float)), ("numel", c_int64)]


# name -> (restype, argtypes); must list every symbol include/css_hip.h declares
# (tests/test_cabi_symbols.py parses the header and checks this table and the .so).
PROTOTYPES = {
    "css_version": (c_char_p, []),
    "css_last_error": (c_char_p, []),
    "css_device_count": (c_int, [POINTER(c_int)]),
    "css_device_info": (c_int, [c_int, POINTER(DevInfo)]),
    "css_index_create": (c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    "css_index_free": (c_int, [c_void_p]),
    "css_index_reset": (c_int, [c_void_p]),
    "css_index_reserve": (c_int, [c_void_p, c_int64]),
    "css_index_remove_rows": (c_int, [c_void_p, c_void_p, POINTER(c_int64)]),
    "css_index_bounds": (c_int, [c_void_p, POINTER(c_float)]),
    "css_index_ntotal": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_dim": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_metric": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_device": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_set_shadow": (c_int, [c_void_p, c_int]),
    "css_index_last_flagged": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_last_swept": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_shadow_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "css_index_set_range_rows": (c_int, [c_void_p, c_int64]),
    "css_index_set_id_base": (c_int, [c_void_p, c_int64]),
    "css_index_set_search_mode": (c_int, [c_void_p, c_int]),
    "css_index_add": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
    "css_index_add_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "css_index_add_synthetic": (c_int, [c_void_p, c_int64, c_uint64, c_int64, c_int, c_void_p]),
    "css_index_export": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "css_index_search": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "css_index_search_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_search_masked": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_search_masked_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "css_index_search_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_search_rows_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "css_index_set_groups": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "css_index_get_groups": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "css_index_search_grouped": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "css_index_last_group_passes": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_set_priors": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "css_index_get_priors": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "css_index_search_prior": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "css_index_search_examples": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                          c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_index_export_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "css_index_kmeans_step": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      POINTER(c_int), POINTER(c_int), c_void_p, c_void_p]),
    "css_index_set_gram_rows": (c_int, [c_void_p, c_int64]),
    "css_index_gram": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "css_index_transform": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p]),
    "css_index_set_terms": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "css_index_get_terms": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "css_index_term_stats": (c_int, [c_void_p, c_void_p, c_int, c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "css_index_set_sigterm_slots": (c_int, [c_void_p, c_int]),
    "css_index_subset_terms": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "css_index_significant_terms": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, POINTER(c_int), POINTER(c_int64), POINTER(c_int64)]),
    "css_index_search_hybrid": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_float, c_float,
                                        c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_index_set_sparse": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "css_index_get_sparse": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "css_index_sparse_rows": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_search_sparse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_search_hybrid_sparse": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_index_set_tokens": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int]),
    "css_index_get_tokens": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "css_index_token_rows": (c_int, [c_void_p, POINTER(c_int64)]),
    "css_index_token_dim": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_drop_tokens": (c_int, [c_void_p]),
    "css_index_set_token_blocks": (c_int, [c_void_p, c_int]),
    "css_index_search_maxsim": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_maxsim_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "css_index_search_maxsim_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "css_index_last_maxsim_passes": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_maxsim_rows_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "css_index_search_rerank_maxsim": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                               c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_index_maxsim_candidates": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                            POINTER(c_int64)]),
    "css_index_search_maxsim_pruned": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                               POINTER(c_int64)]),
    "css_index_set_token_codec": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "css_index_get_token_codec": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_void_p, c_void_p,
                                          c_void_p]),
    "css_index_token_codec_bits": (c_int, [c_void_p, POINTER(c_int)]),
    "css_index_get_token_codes": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "css_index_set_token_codes": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "css_index_search_diverse": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                         c_void_p]),
    "css_index_search_diverse_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                             c_void_p, c_void_p]),
    "css_index_range_search": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_int, c_void_p, POINTER(c_void_p)]),
    "css_range_result_lims": (c_int, [c_void_p, c_void_p]),
    "css_range_result_read": (c_int, [c_void_p, c_void_p, c_void_p]),
    "css_range_result_free": (c_int, [c_void_p]),
    "css_index_facets": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "css_index_last_facet_sweeps": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "css_index_set_facet_lds_entries": (c_int, [c_void_p, c_int64]),
    "css_index_set_attr": (c_int, [c_void_p, c_int, c_int, c_int64, c_int64, c_void_p]),
    "css_index_get_attr": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p]),
    "css_index_attr_type": (c_int, [c_void_p, c_int, POINTER(c_int)]),
    "css_index_drop_attr": (c_int, [c_void_p, c_int]),
    "css_index_where": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, POINTER(c_int64)]),
    "css_index_facets_attr": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_int, c_void_p, c_int, c_int64, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_merge_topk_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "css_merge_topk_packed_dev": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_int,
                                          c_void_p]),
    "css_encoder_create": (c_int, [POINTER(EncoderCfg), c_int, POINTER(c_void_p)]),
    "css_encoder_free": (c_int, [c_void_p]),
    "css_encoder_load_weights": (c_int, [c_void_p, POINTER(Tensor), c_int]),
    "css_encoder_init_synthetic": (c_int, [c_void_p, c_uint64]),
    "css_encoder_export_weight": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "css_encoder_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "css_encoder_forward_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "css_encoder_forward_spans": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p]),
    "css_encoder_forward_spans_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                              c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_encoder_set_head": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_encoder_forward_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "css_encoder_forward_pairs_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                              c_void_p]),
    "css_encoder_set_token_projection": (c_int, [c_void_p, c_void_p, c_int]),
    "css_encoder_token_dim": (c_int, [c_void_p]),
    "css_encoder_forward_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "css_encoder_forward_tokens_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p]),
    "css_encoder_maxsim": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                   c_int, c_void_p]),
    "css_encoder_maxsim_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                       c_int, c_int, c_void_p, c_void_p]),
    "css_encoder_forward_maxsim": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                           c_int, c_void_p, c_void_p]),
    "css_encoder_forward_maxsim_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                               c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "css_encoder_set_mlm_head": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_encoder_vocab_max": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "css_encoder_vocab_max_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "css_encoder_forward_sparse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "css_encoder_forward_sparse_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "css_encoder_debug_read": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    "css_encoder_set_attention_range": (c_int, [c_void_p, c_float]),
    "css_mpnet_rel_bucket": (c_int, [c_int, c_int, c_int]),
    "css_tokenizer_create": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
    "css_tokenizer_free": (c_int, [c_void_p]),
    "css_tokenizer_vocab_size": (c_int, [c_void_p, POINTER(c_int)]),
    "css_tokenizer_encode_batch": (c_int, [c_void_p, c_char_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int]),
    "css_prof_enable": (c_int, [c_int]),
    "css_prof_reset": (c_int, []),
    "css_prof_read": (c_int, [c_char_p, POINTER(c_double), POINTER(c_int64)]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load ``libcss_hip.so`` (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C claude_semantic_search_amd/csrc`. There is no CPU fallback."
        )
    # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Load
    # torch first when it is installed so that exactly one HIP runtime is mapped
    # in the process whichever of the two is imported first by the application.
    try:  # pragma: no cover - depends on the environment
        import torch  # noqa: F401
    except Exception:
        pass
    handle = ctypes.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | os.RTLD_LOCAL if hasattr(os, "RTLD_NOW") else 0)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            if os.environ.get("CSS_HIP_LIB"):  # an A/B build of an older tree (tools/build_variant.sh): newer entry points absent
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return handle


def last_error() -> str:
    return (lib().css_last_error() or b"").decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != CSS_OK:
        raise CssError(rc, last_error())


def device_count() -> int:
    n = c_int(0)
    check(lib().css_device_count(ctypes.byref(n)))
    return int(n.value)


def device_info(device: int = 0) -> dict:
    info = DevInfo()
    check(lib().css_device_info(device, ctypes.byref(info)))
    return {
        "name": info.name.decode(),
        "gcn_arch": info.gcn_arch.decode(),
        "compute_units": info.compute_units,
        "wavefront_size": info.wavefront_size,
        "hbm_total_bytes": info.hbm_total_bytes,
        "hbm_free_bytes": info.hbm_free_bytes,
        "lds_bytes_per_cu": info.lds_bytes_per_cu,
        "clock_mhz": info.clock_mhz,
    }


def prof_enable(on: bool) -> None:
    check(lib().css_prof_enable(1 if on else 0))


def prof_reset() -> None:
    check(lib().css_prof_reset())


def prof_read(kernel: str):
    ms = c_double(0.0)
    n = c_int64(0)
    check(lib().css_prof_read(kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
    return float(ms.value), int(n.value)
