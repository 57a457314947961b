"""parallel-gcn_amd -- Python host glue for the MI355X GCN engine (libpgcn.so).

The product is C++/HIP: kernels + host classes behind the C ABI in include/pgcn.h.  This
module only binds that ABI with ctypes so tests, bench.py and __graft_entry__ can drive it;
it mirrors the reference's host interface for the path (src/main.cpp:9-61,
include/gcn.cuh:79-122): load a dataset with the kept hpdga Parser, build a GCN, call
train_epoch() / eval(split) / run().

There is no CPU fallback: importing this module without the built library raises, and
creating an engine without a HIP device raises PgcnError(PGCN_E_NODEVICE).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PGCN_LIB: another build of the library (A/B experiments); the default is the in-tree build
LIB_PATH = os.environ.get("PGCN_LIB") or os.path.join(HERE, "libpgcn.so")

PGCN_OK = 0
PGCN_E_INVALID = -1
PGCN_E_NOMEM = -2
PGCN_E_IO = -3
PGCN_E_COMM = -4
PGCN_E_NODEVICE = -5
MAX_LAYERS = 16
PGCN_LOAD_WEIGHTS_ONLY = 1
PREDICT_ROWS = 64  # PGCN_PREDICT_ROWS: rows per workgroup of pgcn_predict_rows

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is not built: run `make -C parallel-gcn_amd` "
                      "(or __graft_entry__.build()); there is no fallback path")
lib = ctypes.CDLL(LIB_PATH)

c_int, c_ll, c_float, c_void_p = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p
c_size_t, c_u64, c_double = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_double
P = ctypes.POINTER


class PgcnParams(ctypes.Structure):
    _fields_ = [("num_nodes", c_int), ("input_dim", c_int), ("output_dim", c_int),
                ("n_layers", c_int), ("link_decoder", c_int),
                ("hidden_dims", c_int * MAX_LAYERS),
                ("dropouts", c_float * MAX_LAYERS), ("aggregator", c_int),
                ("root_weight", c_int), ("epochs", c_int), ("readout", c_int),
                ("early_stopping", c_int),
                ("attention_heads", c_int), ("attention_dropout", c_float),
                ("learning_rate", c_float), ("weight_decay", c_float), ("beta1", c_float),
                ("beta2", c_float), ("eps", c_float), ("attention", c_int),
                ("reassociate_last", c_int),
                ("multilabel", c_int), ("seed", ctypes.c_uint), ("layer_norm", c_int), ("residual", c_int)]


class PgcnData(ctypes.Structure):
    _fields_ = [("num_nodes", c_int), ("graph_indptr", P(c_int)), ("graph_indices", P(c_int)),
                ("feat_indptr", P(c_int)), ("feat_indices", P(c_int)),
                ("feat_values", P(c_float)), ("label", P(c_int)), ("split", P(c_int)),
                ("num_pairs", c_int), ("pair_src", P(c_int)), ("pair_dst", P(c_int)),
                ("pair_label", P(c_int)), ("pair_split", P(c_int)),
                ("label_bits", P(ctypes.c_uint32)), ("label_words", c_int),
                ("num_graphs", c_int), ("graph_ptr", P(c_int)), ("graph_label", P(c_int)),
                ("graph_split", P(c_int))]


class PgcnXentFinal(ctypes.Structure):
    """pgcn_xent_final: the loss kernel's fused finish (device pointers as integers)."""
    _fields_ = [("w", c_void_p), ("n_w", c_ll), ("wd", c_float), ("out2", c_void_p),
                ("ctr", c_void_p), ("ring_cap", c_int), ("sums", c_void_p),
                ("ticket", c_void_p), ("part4", c_void_p), ("group", c_int),
                ("gticket", c_void_p), ("gpart4", c_void_p)]


def _sig(name, res, *args):
    if os.environ.get("PGCN_LIB") and not hasattr(lib, name):
        return None  # an A/B build from before this entry point: the bench does not call it
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_sig("pgcn_status_string", ctypes.c_char_p, c_int)
_sig("pgcn_version", c_int)
_sig("pgcn_rng_seed", None, P(c_u64))
_sig("pgcn_rng_seed_glibc", None, ctypes.c_uint, P(c_u64))
_sig("pgcn_rng_jump", None, P(c_u64), c_u64)
_sig("pgcn_rng_jump_table", c_int, c_u64, c_void_p)
_sig("pgcn_graph_create", c_int, c_int, c_void_p, c_void_p, P(c_void_p))
_sig("pgcn_graph_create_values", c_int, c_int, c_void_p, c_void_p, c_void_p, P(c_void_p))
_sig("pgcn_graph_destroy", c_int, c_void_p)
_sig("pgcn_graph_nnz", c_ll, c_void_p)
_sig("pgcn_graphsum", c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p)
_sig("pgcn_gemm", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
     c_int, c_void_p, c_ll, c_ll, c_float, c_void_p)
_sig("pgcn_gemm_tn_workspace", c_size_t, c_int, c_int, c_int)
_sig("pgcn_gemm_tn", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
     c_int, c_void_p, c_ll, c_ll, c_float, c_void_p, c_void_p)
_sig("pgcn_mask_nibbles", c_int, c_void_p, c_ll, c_ll, c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_gemm_xstream", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
     c_void_p, c_int, c_void_p, c_float, c_void_p)
_sig("pgcn_gemm_xstream_dual", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_int, c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p)
_sig("pgcn_gemm_tn_xstream", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p)
_sig("pgcn_gemm_xstream_flat", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_int, c_void_p, c_void_p, c_int, c_void_p, c_ll, c_ll, c_float, c_void_p)
_sig("pgcn_gemm_tn_xstream_flat", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_int, c_void_p, c_ll, c_ll, c_float, c_void_p, c_void_p)
_sig("pgcn_spmm_csr", c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
     c_void_p, c_void_p, c_void_p)
_sig("pgcn_spmm_csc_bwd", c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
     c_float, c_void_p, c_void_p, c_void_p)
_sig("pgcn_csr_transpose", c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p)
_sig("pgcn_dropout_mask", c_int, c_void_p, c_ll, c_ll, c_ll, c_float, c_void_p, c_void_p, c_void_p)
_sig("pgcn_dropout_apply", c_int, c_void_p, c_ll, c_void_p, c_float, c_void_p)
_sig("pgcn_relu_fwd", c_int, c_void_p, c_ll, c_void_p, c_int, c_void_p)
_sig("pgcn_relu_bwd", c_int, c_void_p, c_ll, c_void_p, c_void_p)
_sig("pgcn_residual_fwd", c_int, c_void_p, c_void_p, c_ll, c_void_p)
_sig("pgcn_residual_bwd", c_int, c_void_p, c_void_p, c_ll, c_void_p)
_sig("pgcn_layernorm_fwd", c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p,
     c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p)
_sig("pgcn_layernorm_bwd_workspace", c_size_t, c_int, c_int)
_sig("pgcn_layernorm_bwd", c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
     c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_layernorm_fwd_tail", c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
     c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_ll, c_float, c_void_p)
_sig("pgcn_gat_scores", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
     c_void_p, c_void_p)
_sig("pgcn_gat_fwd", c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p,
     c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_gat_bwd_workspace", c_size_t, c_void_p, c_int)
_sig("pgcn_gat_bwd", c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p,
     c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
     c_void_p, c_void_p)
_sig("pgcn_gat_scores_mh", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
     c_void_p, c_void_p, c_void_p)
_sig("pgcn_gat_fwd_mh", c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p,
     c_int, c_int, c_int, c_void_p, c_ll, c_float, c_void_p, c_void_p)
_sig("pgcn_gat_bwd_workspace_mh", c_size_t, c_void_p, c_int, c_int)
_sig("pgcn_gat_bwd_mh", c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p,
     c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
     c_void_p, c_ll, c_float, c_void_p, c_void_p, c_void_p)
_sig("pgcn_graph_create_mean", c_int, c_int, c_void_p, c_void_p, c_int, P(c_void_p))
_sig("pgcn_agg_max_fwd", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_int, c_void_p)
_sig("pgcn_agg_max_bwd", c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
     c_void_p)
_sig("pgcn_readout_chunk_rows", c_int)
_sig("pgcn_readout_workspace", c_size_t, c_int)
_sig("pgcn_readout_fwd", c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
     c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p)
_sig("pgcn_readout_bwd", c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
     c_int, c_int, c_void_p, c_int, c_void_p)
_sig("pgcn_links_create", c_int, c_int, c_ll, c_void_p, c_void_p, c_void_p, P(c_void_p))
_sig("pgcn_links_destroy", c_int, c_void_p)
_sig("pgcn_link_segment_slots", c_int)
_sig("pgcn_links_slots", c_ll, c_void_p)
_sig("pgcn_link_score_fwd", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p)
_sig("pgcn_link_score_bwd", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
     c_int, c_void_p)
_sig("pgcn_debug_links_incidence", c_int, c_int, c_ll, c_void_p, c_void_p, c_void_p, c_void_p,
     c_void_p, c_void_p)
_sig("pgcn_rank_queries_create", c_int, c_int, c_ll, c_void_p, c_void_p, c_void_p, c_void_p,
     P(c_void_p))
_sig("pgcn_rank_queries_destroy", c_int, c_void_p)
_sig("pgcn_link_rank_tile", None, P(c_int), P(c_int))
_sig("pgcn_link_rank_scores", c_int, c_void_p, c_void_p, c_ll, c_void_p, c_int, c_int, c_void_p,
     c_void_p)
_sig("pgcn_link_rank", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_rank_filter", c_ll, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p,
     c_void_p, c_int, c_int, c_int, P(c_ll), c_void_p, c_void_p, c_void_p, c_void_p)
_sig("pgcn_gcn_link_ranks", c_ll, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_topk_queries_create", c_int, c_int, c_ll, c_void_p, c_void_p, c_void_p, c_int,
     P(c_void_p))
_sig("pgcn_topk_queries_destroy", c_int, c_void_p)
_sig("pgcn_topk_queries_workspace", c_ll, c_void_p)
_sig("pgcn_link_topk_tile", None, P(c_int), P(c_int), P(c_int))
_sig("pgcn_link_topk_splits", c_int, c_ll, c_int)
_sig("pgcn_link_topk_chunk", c_int)
_sig("pgcn_link_topk", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_topk_filter", c_ll, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p,
     c_void_p, c_ll, c_void_p, c_int, c_int, P(c_ll), c_void_p, c_void_p)
_sig("pgcn_gcn_top_links", c_ll, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_params_sizeof", c_int)
_sig("pgcn_xent_blocks", c_int, c_int)
_sig("pgcn_xent_fwd", c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
     c_void_p, c_void_p)
_sig("pgcn_finalize", c_int, c_void_p, c_int, c_int, c_void_p, c_ll, c_float, c_void_p, c_void_p)
_sig("pgcn_adam", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_float, c_float, c_float,
     c_float, c_float, c_int, c_void_p)
_sig("pgcn_adam_step_size", c_float, c_float, c_float, c_float, c_int)
_sig("pgcn_params_default", None, P(PgcnParams))
_sig("pgcn_gcn_create", c_int, P(PgcnParams), P(PgcnData), c_int, P(c_void_p))
_sig("pgcn_comm_unique_id", c_int, c_void_p)
_sig("pgcn_gcn_create_dist", c_int, P(PgcnParams), P(PgcnData), c_int, c_int, c_int, c_void_p,
     P(c_void_p))
_sig("pgcn_gcn_destroy", c_int, c_void_p)
# the caller's host all-gather for the peer-mapped engine (pgcn_allgather_fn)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p)
_sig("pgcn_gcn_create_peer", c_int, P(PgcnParams), P(PgcnData), c_int, c_int, c_int,
     ALLGATHER_FN, c_void_p, P(c_void_p))
_sig("pgcn_loopback_create", c_int, c_int, P(c_void_p))
_sig("pgcn_debug_gcn_create_solo", c_int, P(PgcnParams), P(PgcnData), c_int, c_int, c_int,
     P(c_void_p))
_sig("pgcn_loopback_destroy", c_int, c_void_p)
_sig("pgcn_gcn_create_loopback", c_int, P(PgcnParams), P(PgcnData), c_int, c_int, c_void_p,
     P(c_void_p))
_sig("pgcn_gcn_query", c_ll, c_void_p, ctypes.c_char_p)
_sig("pgcn_gcn_train_epoch", c_int, c_void_p, P(c_float))
_sig("pgcn_gcn_eval", c_int, c_void_p, c_int, P(c_float))
_sig("pgcn_gcn_epoch_async", c_int, c_void_p)
_sig("pgcn_gcn_sync", c_int, c_void_p)
_sig("pgcn_gcn_results", c_int, c_void_p, c_int, P(c_float))
_sig("pgcn_gcn_run", c_int, c_void_p, c_int)
_sig("pgcn_gcn_get_var", c_ll, c_void_p, c_int, c_int, P(c_float))
_sig("pgcn_gcn_num_vars", c_int, c_void_p)
_sig("pgcn_gcn_set_var", c_int, c_void_p, c_int, c_int, c_void_p, c_ll)
_sig("pgcn_gcn_save", c_int, c_void_p, ctypes.c_char_p)
_sig("pgcn_gcn_load", c_int, c_void_p, ctypes.c_char_p, c_int)
_sig("pgcn_checkpoint_info", c_int, ctypes.c_char_p, P(c_ll))
_sig("pgcn_checkpoint_flags", c_int, ctypes.c_char_p)
_sig("pgcn_checkpoint_attention", c_int, ctypes.c_char_p, P(c_int), P(c_float))
_sig("pgcn_checkpoint_sage", c_int, ctypes.c_char_p, P(c_int), P(c_int))
_sig("pgcn_checkpoint_readout", c_int, ctypes.c_char_p, P(c_int), P(c_int))
_sig("pgcn_checkpoint_links", c_int, ctypes.c_char_p, P(c_int), P(c_ll))
_sig("pgcn_gcn_predict_links", c_ll, c_void_p, c_void_p, c_void_p)
_sig("pgcn_gcn_link_counts", c_int, c_void_p, c_int, c_void_p)
_sig("pgcn_gcn_score_pairs", c_int, c_void_p, c_void_p, c_void_p, c_ll, c_void_p)
_sig("pgcn_dataset_set_links", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int)
_sig("pgcn_dataset_load_links", c_int, c_void_p, ctypes.c_char_p, c_int)
_sig("pgcn_gcn_predict", c_ll, c_void_p, c_void_p, c_void_p, c_void_p)
_sig("pgcn_gcn_confusion", c_int, c_void_p, c_int, c_void_p)
_sig("pgcn_predict_rows", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
     c_int, c_void_p)
_sig("pgcn_confusion", c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_bce_fwd", c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
     c_int, c_int, c_void_p, c_void_p)
_sig("pgcn_predict_multilabel_rows", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
     c_void_p, c_int, c_void_p)
_sig("pgcn_multilabel_counts", c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
     c_void_p)
_sig("pgcn_gcn_predict_multilabel", c_ll, c_void_p, c_void_p, c_void_p)
_sig("pgcn_gcn_multilabel_counts", c_int, c_void_p, c_int, c_void_p)
_sig("pgcn_dataset_set_multilabel", c_int, c_void_p, c_void_p, c_int, c_int)
_sig("pgcn_dataset_load_labels", c_int, c_void_p, ctypes.c_char_p, c_int)
_sig("pgcn_dataset_set_graphs", c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int)
_sig("pgcn_dataset_load_graphs", c_int, c_void_p, ctypes.c_char_p, c_int)
_sig("pgcn_gcn_profile", c_int, c_void_p, c_int)
_sig("pgcn_gcn_profile_read", c_int, c_void_p, P(c_double), P(c_ll), P(c_double))
_sig("pgcn_gcn_profile_read_mm", c_int, c_void_p, P(c_double), P(c_ll), P(c_double))
_sig("pgcn_gcn_node_range", c_int, c_void_p, P(c_int), P(c_int))
_sig("pgcn_dataset_load", c_int, ctypes.c_char_p, ctypes.c_char_p, P(c_void_p))
_sig("pgcn_dataset_load_cached", c_int, ctypes.c_char_p, ctypes.c_char_p, P(c_void_p), P(c_int))
_sig("pgcn_dataset_save", c_int, c_void_p, ctypes.c_char_p)
_sig("pgcn_dataset_binarize", c_int, c_void_p)
_sig("pgcn_dataset_load_binary", c_int, ctypes.c_char_p, P(c_void_p))
_sig("pgcn_dataset_synthetic", c_int, c_int, c_int, c_int, c_ll, c_u64, P(c_void_p))
_sig("pgcn_dataset_view", c_int, c_void_p, P(PgcnData), P(c_int), P(c_int))
_sig("pgcn_dataset_free", c_int, c_void_p)
_sig("pgcn_debug_set", c_int, ctypes.c_char_p, c_int)
_sig("pgcn_debug_knob", c_int, c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int))
_sig("pgcn_debug_path_count", c_ll, ctypes.c_char_p, c_int)
_sig("pgcn_debug_empty_launches", c_int, c_int, c_void_p)
_sig("pgcn_debug_exp_check", c_int, c_void_p, c_ll, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_div_check", c_int, c_void_p, c_void_p, c_ll, c_void_p, c_void_p)
_sig("pgcn_debug_ring_slice_rows", c_int)
_sig("pgcn_debug_xent_fwd", c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
     c_int, c_void_p, c_int, P(PgcnXentFinal), c_void_p)
_sig("pgcn_debug_out_xent", c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
     c_void_p, c_void_p, c_void_p, c_int, P(PgcnXentFinal), c_void_p)
_sig("pgcn_debug_finalize_ring", c_int, c_void_p, c_int, c_int, c_void_p, c_ll, c_float,
     c_void_p, c_void_p, c_int, c_void_p, c_void_p)
_sig("pgcn_debug_tn_reduce_blocks_workspace", c_size_t, c_int, c_int, c_int)
_sig("pgcn_debug_tn_reduce_blocks", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int,
     c_void_p)
_sig("pgcn_debug_tn_reduce_one_pass", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
     c_int, c_void_p)
_sig("pgcn_debug_gemm_nib", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
     c_void_p, c_int, c_void_p, c_ll, c_ll, c_float, c_void_p, c_void_p)
_sig("pgcn_debug_gemm_tn_nib", c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
     c_void_p, c_int, c_void_p, c_ll, c_ll, c_float, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_spmm_csr", c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
     c_ll, c_float, c_void_p, c_void_p, c_void_p, c_void_p)
_sig("pgcn_debug_spmm_csc_bwd", c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
     c_void_p, c_void_p, c_ll, c_float, c_void_p, c_void_p, c_ll, c_void_p, c_int, c_void_p)
_sig("pgcn_debug_dropout_mask", c_int, c_void_p, c_ll, c_ll, c_ll, c_float, c_void_p, c_void_p,
     c_int, c_int, c_void_p)
_sig("pgcn_debug_dropout_mask2", c_int, c_void_p, c_ll, c_ll, c_ll, c_float, c_void_p, c_int,
     c_void_p, c_ll, c_ll, c_ll, c_float, c_void_p, c_int, c_void_p, c_void_p)
_sig("pgcn_debug_dropout_apply", c_int, c_void_p, c_ll, c_void_p, c_ll, c_float, c_void_p)
_sig("pgcn_debug_lds_check", c_int, c_int, c_int, c_void_p, c_void_p, c_int, P(ctypes.c_double),
     P(c_ll))
_sig("pgcn_debug_lds_counts", c_ll, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_ll,
     c_void_p)
_sig("pgcn_partition_bounds", c_int, c_int, c_void_p, c_int, c_void_p, P(c_int))
_sig("pgcn_debug_rank_graph", c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
     c_void_p, c_void_p, c_void_p)
_sig("pgcn_partition_subgraph", c_ll, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
     c_void_p, c_void_p)


class PgcnError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        super().__init__(f"{where}: {lib.pgcn_status_string(status).decode()} ({status})")


def check(status, where=""):
    if status != PGCN_OK:
        raise PgcnError(status, where)
    return status


def _ptr(a):
    return a.ctypes.data_as(c_void_p)


KERNEL_PATHS = ("xs_nn_ring", "xs_tn_ring", "xs_nn", "xs_tn", "gs_ring", "gs_gather", "out_xent",
                "gemm_nn", "gemm_tn", "gemm_nn_w", "gemm_tn_w", "gat_fwd", "gat_bwd", "gat_heads",
                "spmm_csr", "spmm_csr_dual", "spmm_csc_256", "spmm_csc_1024", "spmm_tree_256",
                "spmm_tree_1024", "launches", "link_fwd", "link_bwd", "rank_sweep", "rank_filter",
                "topk_sweep", "topk_merge")


def path_counts(reset=False, thread=False):
    """Launch counts of the kernel families since the last reset (pgcn_debug_path_count);
    thread: the calling host thread's launches only (a loopback rank's own)."""
    out = {}
    t = 2 if thread else 0
    for k in KERNEL_PATHS:
        n = lib.pgcn_debug_path_count(k.encode(), t)
        if n < 0:
            raise PgcnError(int(n), "path_count " + k)
        out[k] = int(n)
    if reset:
        lib.pgcn_debug_path_count(None, 1 | t)
    return out


def reset_path_counts(thread=False):
    check(int(lib.pgcn_debug_path_count(None, 3 if thread else 1)), "path_count reset")


# --------------------------------------------------------------------------- data
class Dataset:
    """GCNData (include/gcn.cuh:51-58) owned by libpgcn: the hpdga loader or the synthetic
    reddit-shaped generator.  Arrays are exposed as zero-copy numpy views."""

    def __init__(self, handle):
        self._h = c_void_p(handle)
        self._refresh()

    def _refresh(self):
        self.view = PgcnData()
        fi, fo = c_int(), c_int()
        check(lib.pgcn_dataset_view(self._h, ctypes.byref(self.view), ctypes.byref(fi),
                                    ctypes.byref(fo)), "dataset_view")
        self.input_dim, self.output_dim = fi.value, fo.value
        self.num_nodes = self.view.num_nodes
        n = self.num_nodes

        def arr(p, count, dt):
            if count == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(p, P(ctypes.c_int if dt == np.int32 else c_float)),
                                         shape=(count,))
        self.graph_indptr = arr(self.view.graph_indptr, n + 1, np.int32)
        self.graph_indices = arr(self.view.graph_indices, int(self.graph_indptr[-1]), np.int32)
        self.feat_indptr = arr(self.view.feat_indptr, n + 1, np.int32)
        nnzx = int(self.feat_indptr[-1])
        self.feat_indices = arr(self.view.feat_indices, nnzx, np.int32)
        self.feat_values = arr(self.view.feat_values, nnzx, np.float32)
        self.label = arr(self.view.label, n, np.int32)
        self.split = arr(self.view.split, n, np.int32)
        # multi-label data: the bit matrix [n][label_words] (None for single-label data)
        self.label_words = self.view.label_words
        self.label_bits = None
        if self.view.label_bits and self.label_words:
            self.label_bits = np.ctypeslib.as_array(self.view.label_bits,
                                                    shape=(n, self.label_words))

        # graph-level data: the row ranges, labels and splits of num_graphs graphs (None without)
        self.num_graphs = self.view.num_graphs
        self.graph_ptr = self.graph_label = self.graph_split = None
        if self.num_graphs > 0 and self.view.graph_ptr:
            g = self.num_graphs
            self.graph_ptr = arr(self.view.graph_ptr, g + 1, np.int32)
            self.graph_label = arr(self.view.graph_label, g, np.int32)
            self.graph_split = arr(self.view.graph_split, g, np.int32)

        # pair-level data for link prediction (None without)
        self.num_pairs = self.view.num_pairs
        self.pair_src = self.pair_dst = self.pair_label = self.pair_split = None
        if self.num_pairs > 0 and self.view.pair_src:
            e = self.num_pairs
            self.pair_src = arr(self.view.pair_src, e, np.int32)
            self.pair_dst = arr(self.view.pair_dst, e, np.int32)
            self.pair_label = arr(self.view.pair_label, e, np.int32)
            self.pair_split = arr(self.view.pair_split, e, np.int32)

    def set_links(self, src, dst, labels, splits, embed_dim):
        """Attaches E node pairs for link prediction: src, dst [E] in [0, num_nodes), labels [E]
        1 (a link), 0 (none) or -1 (unlabelled), splits [E] in 0..3; sets output_dim = embed_dim
        (1..128), the width of the node embedding the decoder reads.  The adjacency stays as it
        is: keep validation and test positives out of it."""
        a = [np.ascontiguousarray(x, np.int32) for x in (src, dst, labels, splits)]
        if a[0].ndim != 1 or any(x.shape != a[0].shape for x in a):
            raise ValueError("set_links: src, dst, labels, splits [E]")
        check(lib.pgcn_dataset_set_links(self._h, *(_ptr(x) for x in a), a[0].size, embed_dim),
              "dataset_set_links")
        self._refresh()

    def load_links(self, path, embed_dim):
        """Reads the pair sidecar file (line e: `<src> <dst> <label> <split>`; by convention
        <root>/data/<name>.links) and sets output_dim = embed_dim."""
        check(lib.pgcn_dataset_load_links(self._h, os.fsencode(path), embed_dim),
              f"dataset_load_links {path}")
        self._refresh()

    def set_graphs(self, graph_ptr, labels, splits, num_classes=0):
        """Attaches G graphs as contiguous row ranges: graph_ptr [G + 1] from 0 to num_nodes,
        labels [G] in [0, classes) or -1 (unlabelled), splits [G] in 0..3; sets output_dim = the
        class count (num_classes, or max label + 1 when 0)."""
        gp = np.ascontiguousarray(graph_ptr, np.int32)
        lb = np.ascontiguousarray(labels, np.int32)
        sp = np.ascontiguousarray(splits, np.int32)
        if gp.ndim != 1 or gp.size < 2 or lb.shape != (gp.size - 1,) or sp.shape != lb.shape:
            raise ValueError("set_graphs: graph_ptr [G + 1], labels [G], splits [G]")
        check(lib.pgcn_dataset_set_graphs(self._h, _ptr(gp), _ptr(lb), _ptr(sp), lb.size,
                                          num_classes), "dataset_set_graphs")
        self._refresh()

    def load_graphs(self, path, num_classes=0):
        """Reads the graph-level sidecar file (line g: `<rows> <label> <split>`; by convention
        <root>/data/<name>.graphs); num_classes 0: max label + 1."""
        check(lib.pgcn_dataset_load_graphs(self._h, os.fsencode(path), num_classes),
              f"dataset_load_graphs {path}")
        self._refresh()

    def set_multilabel(self, Y):
        """Attaches the label matrix Y (bool [num_nodes][C], 1 <= C <= 128) and sets output_dim =
        C; labelled nodes (label >= 0) stay labelled."""
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.shape[0] != self.num_nodes:
            raise ValueError("set_multilabel: Y must be [num_nodes][C]")
        bits = pack_label_bits(Y)
        check(lib.pgcn_dataset_set_multilabel(self._h, _ptr(bits), bits.shape[1], Y.shape[1]),
              "dataset_set_multilabel")
        self._refresh()

    def load_labels(self, path, num_classes=0):
        """Reads the multi-label sidecar file (line i: the class ids of node i; by convention
        <root>/data/<name>.labels); num_classes 0: max id + 1."""
        check(lib.pgcn_dataset_load_labels(self._h, os.fsencode(path), num_classes),
              f"dataset_load_labels {path}")
        self._refresh()

    @staticmethod
    def load(root, name):
        """Parser(&params, &data, name).parse() with data/<name>.* under root."""
        h = c_void_p()
        check(lib.pgcn_dataset_load(root.encode(), name.encode(), ctypes.byref(h)),
              f"Cannot read input: {name}")
        return Dataset(h.value)

    @staticmethod
    def load_cached(root, name):
        """load() through the binary cache data/<name>.pgcnbin (written on a miss).
        Returns (dataset, from_cache)."""
        h, hit = c_void_p(), c_int()
        check(lib.pgcn_dataset_load_cached(root.encode(), name.encode(), ctypes.byref(h),
                                           ctypes.byref(hit)), f"Cannot read input: {name}")
        return Dataset(h.value), bool(hit.value)

    def binarize(self):
        """PART2 NO_FEATURE (src/parser.cpp:100-104): every feature value becomes 1.0 (the
        arrays of this object are views, so they change in place)."""
        check(lib.pgcn_dataset_binarize(self._h), "dataset_binarize")

    def save(self, path):
        check(lib.pgcn_dataset_save(self._h, path.encode()), f"dataset_save {path}")

    @staticmethod
    def load_binary(path):
        h = c_void_p()
        check(lib.pgcn_dataset_load_binary(path.encode(), ctypes.byref(h)),
              f"dataset_load_binary {path}")
        return Dataset(h.value)

    @staticmethod
    def synthetic(n, f, c, undirected_edges, seed=1):
        h = c_void_p()
        check(lib.pgcn_dataset_synthetic(n, f, c, undirected_edges, seed, ctypes.byref(h)),
              "dataset_synthetic")
        return Dataset(h.value)

    def __del__(self):
        # (at interpreter exit the module's globals may already be gone: nothing to free then)
        if getattr(self, "_h", None) and self._h.value and lib is not None:
            lib.pgcn_dataset_free(self._h)
            self._h = c_void_p()


def pack_label_bits(Y):
    """bool [n][C] -> the uint32 bit matrix [n][ceil(C / 32)] (bit j % 32 of word j / 32)."""
    Y = np.asarray(Y).astype(bool)
    n, c = Y.shape
    words = (c + 31) // 32
    pad = np.zeros((n, words * 32), np.uint8)
    pad[:, :c] = Y
    return np.ascontiguousarray(
        np.packbits(pad.reshape(n, words, 32), axis=2, bitorder="little").view("<u4")
        .reshape(n, words).astype(np.uint32))


def unpack_label_bits(bits, c):
    """The inverse: uint32 [n][words] -> bool [n][c]."""
    bits = np.ascontiguousarray(bits, dtype="<u4")
    n = bits.shape[0]
    return np.unpackbits(bits.view(np.uint8).reshape(n, -1), axis=1,
                         bitorder="little")[:, :c].astype(bool)


def f1_scores(counts):
    """(micro-F1, macro-F1) from per-class counts [3][C] = tp, fp, fn (summed over the ranks).
    A class with no positives and no predictions (2 tp + fp + fn == 0) has F1 0."""
    tp, fp, fn = (np.asarray(counts, np.float64)[k] for k in range(3))
    den = 2 * tp + fp + fn
    per = np.divide(2 * tp, den, out=np.zeros_like(den), where=den > 0)
    tot = den.sum()
    return (float(2 * tp.sum() / tot) if tot > 0 else 0.0), float(per.mean())


class Links:
    """A pair index on the device (pgcn_links): n_pairs pairs (src, dst) over n_nodes nodes; the
    pairs with select >= 0 (all when None) enter the backward's incidence index."""

    def __init__(self, n_nodes, src, dst, select=None):
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        if src.ndim != 1 or dst.shape != src.shape:
            raise ValueError("Links: src [E], dst [E]")
        sel = None if select is None else np.ascontiguousarray(select, np.int32)
        if sel is not None and sel.shape != src.shape:
            raise ValueError("Links: select [E]")
        h = c_void_p()
        check(lib.pgcn_links_create(n_nodes, src.size, _ptr(src), _ptr(dst),
                                    _ptr(sel) if sel is not None else None, ctypes.byref(h)),
              "links_create")
        self._h, self.n_nodes, self.n_pairs = h, n_nodes, int(src.size)

    @property
    def handle(self):
        return self._h

    def slots(self):
        return int(lib.pgcn_links_slots(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value and lib is not None:
            lib.pgcn_links_destroy(self._h)
            self._h = c_void_p()

    __del__ = close


def links_incidence(n_nodes, src, dst, select=None):
    """Host-only: (ptr [n_nodes + 1], pair, other) -- the incidence index pgcn_links_create
    builds (pgcn_debug_links_incidence)."""
    src = np.ascontiguousarray(src, np.int32)
    dst = np.ascontiguousarray(dst, np.int32)
    sel = None if select is None else np.ascontiguousarray(select, np.int32)
    ps = _ptr(sel) if sel is not None else None
    ptr = np.zeros(n_nodes + 1, np.int32)
    check(lib.pgcn_debug_links_incidence(n_nodes, src.size, _ptr(src), _ptr(dst), ps, _ptr(ptr),
                                         None, None), "debug_links_incidence")
    pair, other = np.zeros(ptr[-1], np.int32), np.zeros(ptr[-1], np.int32)
    check(lib.pgcn_debug_links_incidence(n_nodes, src.size, _ptr(src), _ptr(dst), ps, _ptr(ptr),
                                         _ptr(pair), _ptr(other)), "debug_links_incidence")
    return ptr, pair, other


class RankQueries:
    """A ranking query set on the device (pgcn_rank_queries): per query an anchor and a target
    over n_nodes nodes and, with filter_ptr [Q + 1] / filter_idx, a strictly ascending list of
    candidates to leave out (never the target)."""

    def __init__(self, n_nodes, anchor, target, filter_ptr=None, filter_idx=None):
        anchor = np.ascontiguousarray(anchor, np.int32)
        target = np.ascontiguousarray(target, np.int32)
        if anchor.ndim != 1 or target.shape != anchor.shape:
            raise ValueError("RankQueries: anchor [Q], target [Q]")
        fp = fi = None
        if filter_ptr is not None:
            fp = np.ascontiguousarray(filter_ptr, np.int64)
            fi = np.ascontiguousarray(filter_idx if filter_idx is not None else [], np.int32)
            if fp.shape != (anchor.size + 1,) or fi.ndim != 1 or (fp.size and fp[-1] != fi.size):
                raise ValueError("RankQueries: filter_ptr [Q + 1], filter_idx [filter_ptr[Q]]")
        h = c_void_p()
        check(lib.pgcn_rank_queries_create(n_nodes, anchor.size, _ptr(anchor), _ptr(target),
                                           _ptr(fp) if fp is not None else None,
                                           _ptr(fi) if fi is not None else None, ctypes.byref(h)),
              "rank_queries_create")
        self._h, self.n_nodes, self.n_queries = h, n_nodes, int(anchor.size)
        self.filtered = fp is not None

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) and self._h.value and lib is not None:
            lib.pgcn_rank_queries_destroy(self._h)
            self._h = c_void_p()

    __del__ = close


def link_rank_tile():
    """(queries per workgroup, candidates per tile) of the ranking sweep (pgcn_link_rank_tile)."""
    tq, tc = c_int(), c_int()
    lib.pgcn_link_rank_tile(ctypes.byref(tq), ctypes.byref(tc))
    return tq.value, tc.value


def rank_filter(n_nodes, indptr, indices, pair_src, pair_dst, pair_label, pair_split, split,
                side="dst", filtered=True):
    """Host-only: (anchor, target, ptr int64 [Q + 1], idx) -- the query set GCN.link_ranks builds
    for `split` (pgcn_debug_rank_filter): the split's positive pairs in pair order and, filtered,
    per query the ascending union of the anchor, its neighbours in the pattern and its known links
    of every split, minus the target."""
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    a = [np.ascontiguousarray(x, np.int32) for x in (pair_src, pair_dst, pair_label, pair_split)]
    if any(x.ndim != 1 or x.shape != a[0].shape for x in a):
        raise ValueError("rank_filter: pair_src, pair_dst, pair_label, pair_split [E]")
    args = (n_nodes, _ptr(indptr), _ptr(indices), a[0].size, *(_ptr(x) for x in a), split,
            RANK_SIDES[side], 1 if filtered else 0)
    nf = c_ll()
    q = lib.pgcn_debug_rank_filter(*args, ctypes.byref(nf), None, None, None, None)
    if q < 0:
        raise PgcnError(int(q), "debug_rank_filter")
    anchor, target = np.zeros(q, np.int32), np.zeros(q, np.int32)
    ptr, idx = np.zeros(q + 1, np.int64), np.zeros(nf.value, np.int32)
    got = lib.pgcn_debug_rank_filter(*args, ctypes.byref(nf), _ptr(anchor), _ptr(target),
                                     _ptr(ptr), _ptr(idx))
    if got < 0:
        raise PgcnError(int(got), "debug_rank_filter")
    return anchor, target, ptr, idx


RANK_SIDES = {"dst": 0, "src": 1, 0: 0, 1: 1}


class TopKQueries:
    """A top-K query set on the device (pgcn_topk_queries): per query an anchor over n_nodes nodes
    and, with exclude_ptr [Q + 1] / exclude_idx, a strictly ascending list of candidates to leave
    out (it may hold the anchor); k results per query.  It owns the workspace of pgcn_link_topk."""

    def __init__(self, n_nodes, anchor, exclude_ptr=None, exclude_idx=None, k=10):
        anchor = np.ascontiguousarray(anchor, np.int32)
        if anchor.ndim != 1:
            raise ValueError("TopKQueries: anchor [Q]")
        xp = xi = None
        if exclude_ptr is not None:
            xp = np.ascontiguousarray(exclude_ptr, np.int64)
            xi = np.ascontiguousarray(exclude_idx if exclude_idx is not None else [], np.int32)
            if xp.shape != (anchor.size + 1,) or xi.ndim != 1 or (xp.size and xp[-1] != xi.size):
                raise ValueError("TopKQueries: exclude_ptr [Q + 1], exclude_idx [exclude_ptr[Q]]")
        h = c_void_p()
        check(lib.pgcn_topk_queries_create(n_nodes, anchor.size, _ptr(anchor),
                                           _ptr(xp) if xp is not None else None,
                                           _ptr(xi) if xi is not None else None, int(k),
                                           ctypes.byref(h)), "topk_queries_create")
        self._h, self.n_nodes, self.n_queries, self.k = h, n_nodes, int(anchor.size), int(k)
        self.filtered = xp is not None

    @property
    def handle(self):
        return self._h

    @property
    def workspace(self):
        """Device bytes of workspace the handle owns."""
        return int(lib.pgcn_topk_queries_workspace(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value and lib is not None:
            lib.pgcn_topk_queries_destroy(self._h)
            self._h = c_void_p()

    __del__ = close


def link_topk_tile():
    """(queries per workgroup, candidates per tile, largest k) of the top-K sweep
    (pgcn_link_topk_tile)."""
    tq, tc, km = c_int(), c_int(), c_int()
    lib.pgcn_link_topk_tile(ctypes.byref(tq), ctypes.byref(tc), ctypes.byref(km))
    return tq.value, tc.value, km.value


def link_topk_splits(n_queries, n_nodes):
    """Candidate splits of the top-K sweep's grid for (n_queries, n_nodes): host only."""
    return int(lib.pgcn_link_topk_splits(int(n_queries), int(n_nodes)))


def link_topk_chunk():
    """Queries GCN.top_links hands to one top-K call (pgcn_link_topk_chunk)."""
    return int(lib.pgcn_link_topk_chunk())


def topk_filter(n_nodes, indptr, indices, pair_src, pair_dst, pair_label, pair_split, nodes,
                side="dst", filtered=True):
    """Host-only: (ptr int64 [m + 1], idx) -- the exclude lists GCN.top_links builds for `nodes`
    (pgcn_debug_topk_filter): filtered, per node the ascending union of the node, its neighbours in
    the pattern and its known links of every split (rank_filter's list with the target left in)."""
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    a = [np.ascontiguousarray(x, np.int32) for x in (pair_src, pair_dst, pair_label, pair_split)]
    if any(x.ndim != 1 or x.shape != a[0].shape for x in a):
        raise ValueError("topk_filter: pair_src, pair_dst, pair_label, pair_split [E]")
    nodes = np.ascontiguousarray(nodes, np.int32)
    if nodes.ndim != 1:
        raise ValueError("topk_filter: nodes [m]")
    args = (n_nodes, _ptr(indptr), _ptr(indices), a[0].size, *(_ptr(x) for x in a), nodes.size,
            _ptr(nodes), RANK_SIDES[side], 1 if filtered else 0)
    nx = c_ll()
    m = lib.pgcn_debug_topk_filter(*args, ctypes.byref(nx), None, None)
    if m < 0:
        raise PgcnError(int(m), "debug_topk_filter")
    ptr, idx = np.zeros(nodes.size + 1, np.int64), np.zeros(nx.value, np.int32)
    got = lib.pgcn_debug_topk_filter(*args, ctypes.byref(nx), _ptr(ptr), _ptr(idx))
    if got < 0:
        raise PgcnError(int(got), "debug_topk_filter")
    return ptr, idx


def rank_from_counts(greater, equal, ties="mean"):
    """float64 ranks from link_ranks' counts: 'optimistic' greater + 1, 'pessimistic'
    greater + equal + 1, 'mean' greater + equal / 2 + 1."""
    g, e = np.asarray(greater, np.float64), np.asarray(equal, np.float64)
    if ties == "optimistic":
        return g + 1.0
    if ties == "pessimistic":
        return g + e + 1.0
    if ties == "mean":
        return g + e / 2.0 + 1.0
    raise ValueError("ties must be 'mean', 'optimistic' or 'pessimistic'")


def mrr(ranks):
    """Mean reciprocal rank (nan without queries)."""
    r = np.asarray(ranks, np.float64).ravel()
    return float((1.0 / r).mean()) if r.size else float("nan")


def hits_at(ranks, k):
    """The share of queries ranked at or above position k (nan without queries)."""
    r = np.asarray(ranks, np.float64).ravel()
    return float((r <= k).mean()) if r.size else float("nan")


def link_auc(scores, labels):
    """Area under the ROC curve of `scores` against labels in {0, 1} (-1: unlabelled, skipped):
    rank-based (Mann-Whitney), tied scores sharing their average rank.  nan when a class is
    empty."""
    s = np.asarray(scores, np.float64).ravel()
    y = np.asarray(labels).ravel()
    keep = y >= 0
    s, y = s[keep], y[keep]
    pos, neg = int((y == 1).sum()), int((y == 0).sum())
    if pos == 0 or neg == 0:
        return float("nan")
    order = np.argsort(s, kind="stable")
    ss = s[order]
    start = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]])  # the first of every run of equals
    end = np.r_[start[1:], ss.size]
    avg = (start + end + 1) / 2.0  # ranks from 1: the mean of start + 1 .. end
    rank = np.empty(s.size, np.float64)
    rank[order] = np.repeat(avg, end - start)
    return float((rank[y == 1].sum() - pos * (pos + 1) / 2.0) / (pos * neg))


def sample_negative_pairs(ds, src, ratio=1, seed=0):
    """Negative pairs for link prediction, on the host: for every entry of `src`, `ratio` pairs
    (src, dst) with dst drawn uniformly from the nodes, redrawn while it is src itself or a
    neighbour of src in ds's adjacency (either direction).  Deterministic in `seed`.  Returns
    (src int32 [len(src) * ratio], dst int32 [the same])."""
    n = ds.num_nodes
    indptr, indices = np.asarray(ds.graph_indptr), np.asarray(ds.graph_indices)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices.astype(np.int64)
    edges = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))
    s = np.repeat(np.asarray(src, np.int64).ravel(), int(ratio))
    if s.size and (s.min() < 0 or s.max() >= n):
        raise ValueError("sample_negative_pairs: src out of range")
    rng = np.random.default_rng(seed)
    d = rng.integers(0, n, s.size)
    for _ in range(1000):
        bad = np.flatnonzero((d == s) | np.isin(s * n + d, edges))
        if bad.size == 0:
            return s.astype(np.int32), d.astype(np.int32)
        d[bad] = rng.integers(0, n, bad.size)
    raise ValueError("sample_negative_pairs: a source node is adjacent to every other node")


AGGREGATORS = {None: 0, "mean": 1, "max": 2}
READOUTS = {None: 0, "sum": 1, "mean": 2, "max": 3}
LINK_DECODERS = {None: 0, "dot": 1}


def make_params(ds, hidden_dims=(16,), dropouts=(0.5, 0.5), epochs=100, early_stopping=0,
                learning_rate=0.01, weight_decay=5e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                reassociate_last=True, seed=0, residual=False, layer_norm=False,
                multilabel=False, attention=False, attention_heads=1, attention_dropout=0.0,
                aggregator=None, root_weight=False, readout=None, link_decoder=None):
    """aggregator: None (GCN's Â), "mean" or "max" (GraphSAGE layers); root_weight: the layer's
    own row through its own half of a [d_in][2 d_l] weight (with an aggregator only).
    readout: None (node classification), "sum", "mean" or "max": graph classification over the
    graphs attached with Dataset.set_graphs / load_graphs (not with multilabel).
    link_decoder: None or "dot": link prediction over the pairs attached with Dataset.set_links /
    load_links, output_dim being the embedding width (not with multilabel or readout)."""
    if link_decoder not in LINK_DECODERS:
        raise ValueError("link_decoder must be 'dot' or None")
    if LINK_DECODERS[link_decoder] and (multilabel or READOUTS.get(readout)):
        raise ValueError("link_decoder cannot be combined with multilabel or readout")
    if readout not in READOUTS:
        raise ValueError(f"readout must be one of {sorted(k for k in READOUTS if k)} or None")
    if READOUTS[readout] and multilabel:
        raise ValueError("readout cannot be combined with multilabel")
    if aggregator not in AGGREGATORS:
        raise ValueError(f"aggregator must be one of {sorted(k for k in AGGREGATORS if k)} or None")
    if root_weight and not AGGREGATORS[aggregator]:
        raise ValueError("root_weight needs aggregator='mean' or 'max'")
    if attention and AGGREGATORS[aggregator]:
        raise ValueError("an aggregator cannot be combined with attention")
    p = PgcnParams()
    lib.pgcn_params_default(ctypes.byref(p))
    p.aggregator = AGGREGATORS[aggregator]
    p.root_weight = 1 if root_weight else 0
    p.attention = 1 if attention else 0
    p.attention_heads, p.attention_dropout = attention_heads, attention_dropout
    p.multilabel = 1 if multilabel else 0
    p.readout = READOUTS[readout]
    p.link_decoder = LINK_DECODERS[link_decoder]
    p.residual = 1 if residual else 0
    p.layer_norm = 1 if layer_norm else 0
    p.reassociate_last = 1 if reassociate_last else 0
    p.seed = seed
    p.num_nodes, p.input_dim, p.output_dim = ds.num_nodes, ds.input_dim, ds.output_dim
    p.n_layers = len(hidden_dims) + 1
    assert len(dropouts) == p.n_layers
    for i, h in enumerate(hidden_dims):
        p.hidden_dims[i] = h
    for i, d in enumerate(dropouts):
        p.dropouts[i] = d
    p.epochs, p.early_stopping = epochs, early_stopping
    p.learning_rate, p.weight_decay, p.beta1, p.beta2, p.eps = (learning_rate, weight_decay,
                                                               beta1, beta2, eps)
    return p


# --------------------------------------------------------------------------- engine
class GCN:
    """GCN(params, data) of include/gcn.cuh:79-122 on one GPU, or the edge-cut variant when
    rank/world/unique_id are given (one process per GPU)."""

    def __init__(self, params, ds, device=0, rank=None, world=None, unique_id=None,
                 loopback=None, solo=False, allgather=None):
        self.ds = ds  # keep the host data alive while the engine is built
        h = c_void_p()
        self._ag = None
        if allgather is not None:
            # peer-mapped exchange (pgcn_gcn_create_peer): allgather(bytes) -> [bytes of every
            # rank], called at creation and at close (kept alive with the engine)
            self._ag = peer_allgather_fn(allgather)
            check(lib.pgcn_gcn_create_peer(ctypes.byref(params), ctypes.byref(ds.view), device,
                                           rank, world, self._ag, None, ctypes.byref(h)),
                  "gcn_create_peer")
        elif solo:  # timing only: rank `rank` of `world` with no peers (pgcn_debug_gcn_create_solo)
            check(lib.pgcn_debug_gcn_create_solo(ctypes.byref(params), ctypes.byref(ds.view),
                                                 device, rank, world, ctypes.byref(h)),
                  "gcn_create_solo")
        elif loopback is not None:
            check(lib.pgcn_gcn_create_loopback(ctypes.byref(params), ctypes.byref(ds.view),
                                               device, rank, loopback._h, ctypes.byref(h)),
                  "gcn_create_loopback")
        elif world is None:
            check(lib.pgcn_gcn_create(ctypes.byref(params), ctypes.byref(ds.view), device,
                                      ctypes.byref(h)), "gcn_create")
        else:
            uid = ctypes.create_string_buffer(bytes(unique_id), 128)
            check(lib.pgcn_gcn_create_dist(ctypes.byref(params), ctypes.byref(ds.view), device,
                                           rank, world, uid, ctypes.byref(h)), "gcn_create_dist")
        self._h = h
        self.params = params

    def train_epoch(self):
        out = (c_float * 2)()
        check(lib.pgcn_gcn_train_epoch(self._h, out), "train_epoch")
        return out[0], out[1]

    def eval(self, split):
        out = (c_float * 2)()
        check(lib.pgcn_gcn_eval(self._h, split, out), "eval")
        return out[0], out[1]

    def epoch_async(self):
        check(lib.pgcn_gcn_epoch_async(self._h), "epoch_async")

    def sync(self):
        check(lib.pgcn_gcn_sync(self._h), "sync")

    def results(self, n):
        """The last min(n, epochs run, 1024) epoch lines [train_loss, train_acc, val_loss,
        val_acc], oldest first."""
        out = np.zeros(4 * max(n, 0), np.float32)
        rows = lib.pgcn_gcn_results(self._h, n, out.ctypes.data_as(P(c_float)))
        if rows < 0:
            raise PgcnError(rows, "results")
        return out[:4 * rows].reshape(rows, 4)

    def run(self, verbose=True):
        check(lib.pgcn_gcn_run(self._h, 1 if verbose else 0), "run")

    def num_vars(self):
        return lib.pgcn_gcn_num_vars(self._h)

    def get_var(self, idx, which=0):
        n = lib.pgcn_gcn_get_var(self._h, idx, which, None)
        if n < 0:
            raise PgcnError(int(n), "get_var")
        out = np.zeros(n, np.float32)
        if n:
            lib.pgcn_gcn_get_var(self._h, idx, which, out.ctypes.data_as(P(c_float)))
        return out

    def set_var(self, idx, values, which=0):
        """Writes a weight variable (get_var's layout and count); anything else is refused."""
        a = np.ascontiguousarray(values, np.float32).ravel()
        check(lib.pgcn_gcn_set_var(self._h, idx, which, _ptr(a), a.size), "set_var")

    def save(self, path):
        """The whole training state to one checkpoint file (pgcn_gcn_save)."""
        check(lib.pgcn_gcn_save(self._h, os.fsencode(path)), f"save {path}")

    def load(self, path, weights_only=False):
        """Resume from a checkpoint (bit-exact continuation), or take only its weights."""
        check(lib.pgcn_gcn_load(self._h, os.fsencode(path),
                                PGCN_LOAD_WEIGHTS_ONLY if weights_only else 0), f"load {path}")

    def predict(self, probs=False):
        """(classes int32 [rows], confidences float32 [rows]) of this rank's rows from an
        eval-mode forward; with probs=True also the softmax rows [rows, output_dim].  A readout
        engine: one row per graph."""
        a, b = self.node_range()
        n, c = b - a, self.params.output_dim
        if self.params.readout:  # one row per graph
            n = self.query("num_graphs")
        cls, conf = np.zeros(n, np.int32), np.zeros(n, np.float32)
        pr = np.zeros((n, c), np.float32) if probs else None
        got = lib.pgcn_gcn_predict(self._h, _ptr(cls), _ptr(conf), _ptr(pr) if probs else None)
        if got < 0:
            raise PgcnError(int(got), "predict")
        assert got == n
        return (cls, conf, pr) if probs else (cls, conf)

    def confusion(self, split):
        """counts[t, p]: this rank's rows of `split` with label t predicted p (int64)."""
        c = self.params.output_dim
        out = np.zeros((c, c), np.int64)
        check(lib.pgcn_gcn_confusion(self._h, split, _ptr(out)), "confusion")
        return out

    def predict_multilabel(self, probs=False):
        """bool [rows][output_dim] of this rank's rows (logit > 0) from an eval-mode forward of a
        multi-label engine; with probs=True also the sigmoid rows (float32)."""
        a, b = self.node_range()
        n, c = b - a, self.params.output_dim
        bits = np.zeros((n, (c + 31) // 32), np.uint32)
        pr = np.zeros((n, c), np.float32) if probs else None
        got = lib.pgcn_gcn_predict_multilabel(self._h, _ptr(bits), _ptr(pr) if probs else None)
        if got < 0:
            raise PgcnError(int(got), "predict_multilabel")
        assert got == n
        pred = unpack_label_bits(bits, c)
        return (pred, pr) if probs else pred

    def multilabel_counts(self, split):
        """counts[3, C] (int64): per class tp, fp, fn over this rank's rows of `split`; add the
        ranks' arrays, then f1_scores()."""
        out = np.zeros((3, self.params.output_dim), np.int64)
        check(lib.pgcn_gcn_multilabel_counts(self._h, split, _ptr(out)), "multilabel_counts")
        return out

    def predict_links(self, probs=False):
        """float32 [num_pairs]: the scores of a link engine's pairs from an eval-mode forward; with
        probs=True also their sigmoids."""
        n = self.query("num_pairs")
        sc = np.zeros(n, np.float32)
        pr = np.zeros(n, np.float32) if probs else None
        got = lib.pgcn_gcn_predict_links(self._h, _ptr(sc), _ptr(pr) if probs else None)
        if got < 0:
            raise PgcnError(int(got), "predict_links")
        assert got == n
        return (sc, pr) if probs else sc

    def link_counts(self, split):
        """int64 [3]: tp, fp, fn over `split`'s labelled pairs (predicted a link iff score > 0)."""
        out = np.zeros(3, np.int64)
        check(lib.pgcn_gcn_link_counts(self._h, split, _ptr(out)), "link_counts")
        return out

    def link_ranks(self, split, side="dst", filtered=True):
        """(greater, equal) int64 [Q]: for `split`'s Q positive pairs in pair order, the candidates
        scoring above / exactly the true endpoint from an eval-mode forward (side 'dst': the
        destination is ranked among all nodes, 'src': the source; filtered: the anchor, its
        neighbours and its known links do not compete).  See rank_from_counts, mrr, hits_at."""
        if side not in RANK_SIDES:
            raise ValueError("side must be 'dst' or 'src'")
        args = (self._h, split, RANK_SIDES[side], 1 if filtered else 0)
        q = lib.pgcn_gcn_link_ranks(*args, None, None)
        if q < 0:
            raise PgcnError(int(q), "link_ranks")
        greater, equal = np.zeros(q, np.int64), np.zeros(q, np.int64)
        got = lib.pgcn_gcn_link_ranks(*args, _ptr(greater), _ptr(equal))
        if got < 0:
            raise PgcnError(int(got), "link_ranks")
        assert got == q
        return greater, equal

    def top_links(self, nodes, k=10, side="dst", filtered=True):
        """(idx int32 [m][k], scores float32 [m][k]): per node of `nodes` the k nodes with the
        highest rank score against it from an eval-mode forward, ties to the lower index (side
        'dst': destinations for the node as a source, 'src': sources for it as a destination;
        filtered: the node, its neighbours and its known links are left out).  Rows with fewer than
        k candidates end in idx -1, score -inf.  The training state is untouched."""
        if side not in RANK_SIDES:
            raise ValueError("side must be 'dst' or 'src'")
        nodes = np.ascontiguousarray(nodes, np.int32)
        if nodes.ndim != 1:
            raise ValueError("top_links: nodes [m]")
        k = int(k)
        idx = np.zeros((nodes.size, max(k, 0)), np.int32)
        sc = np.zeros((nodes.size, max(k, 0)), np.float32)
        got = lib.pgcn_gcn_top_links(self._h, _ptr(nodes), nodes.size, k, RANK_SIDES[side],
                                     1 if filtered else 0, _ptr(idx), _ptr(sc))
        if got < 0:
            raise PgcnError(int(got), "top_links")
        return idx, sc

    def score_pairs(self, src, dst):
        """float32 [m]: the decoder's scores of caller-given candidate pairs from the same
        eval-mode forward; the training state is untouched."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        if src.ndim != 1 or dst.shape != src.shape:
            raise ValueError("score_pairs: src [m], dst [m]")
        out = np.zeros(src.size, np.float32)
        check(lib.pgcn_gcn_score_pairs(self._h, _ptr(src), _ptr(dst), src.size, _ptr(out)),
              "score_pairs")
        return out

    def profile(self, on):
        check(lib.pgcn_gcn_profile(self._h, 1 if on else 0), "profile")

    def profile_read(self):
        ms, calls, byts = c_double(), c_ll(), c_double()
        check(lib.pgcn_gcn_profile_read(self._h, ctypes.byref(ms), ctypes.byref(calls),
                                        ctypes.byref(byts)), "profile_read")
        return ms.value, calls.value, byts.value

    def profile_read_mm(self):
        """(ms, launches, flops) of the profiled XW contractions (MFMA kernels)."""
        ms, calls, fl = c_double(), c_ll(), c_double()
        check(lib.pgcn_gcn_profile_read_mm(self._h, ctypes.byref(ms), ctypes.byref(calls),
                                           ctypes.byref(fl)), "profile_read_mm")
        return ms.value, calls.value, fl.value

    def query(self, key):
        """Engine facts: world, rank, comm (0 none / 1 RCCL / 2 loopback), reassociated,
        graph_symmetric, graphsum_lds, epochs, adam_steps, norm_layers, fused_norm_tails, ..."""
        v = lib.pgcn_gcn_query(self._h, key.encode())
        if v < 0:
            raise PgcnError(int(v), f"query {key}")
        return int(v)

    def node_range(self):
        a, b = c_int(), c_int()
        lib.pgcn_gcn_node_range(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def close(self):
        if self._h and self._h.value:
            lib.pgcn_gcn_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoopbackGroup:
    """`world` in-process edge-cut ranks on one device (pgcn_loopback_create).  Create the
    engines with GCN(..., rank=r, loopback=group), each from its own thread (see run_ranks)."""

    def __init__(self, world):
        h = c_void_p()
        check(lib.pgcn_loopback_create(world, ctypes.byref(h)), "loopback_create")
        self._h = h
        self.world = world

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib.pgcn_loopback_destroy(self._h)
            self._h = c_void_p()


def peer_allgather_fn(allgather):
    """A pgcn_allgather_fn over a Python all-gather: allgather(data: bytes) -> list of every
    rank's bytes in rank order (torch.distributed, a TCP store, ...)."""
    def cb(mine, nbytes, out, user):
        try:
            parts = allgather(ctypes.string_at(mine, nbytes))
            buf = b"".join(parts)
            if len(buf) != nbytes * len(parts):
                return -1
            ctypes.memmove(out, buf, len(buf))
            return 0
        except Exception:  # noqa: BLE001 -- reported to the engine as a failed all-gather
            return -1
    return ALLGATHER_FN(cb)


def torch_allgather(group=None):
    """allgather(bytes) over torch.distributed (gloo: CPU tensors)."""
    import torch
    import torch.distributed as dist

    def ag(data):
        n = dist.get_world_size(group)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = [torch.empty_like(t) for _ in range(n)]
        dist.all_gather(out, t, group=group)
        return [bytes(o.numpy().tobytes()) for o in out]
    return ag


def run_ranks(world, fn):
    """Calls fn(rank) for every rank in its own thread (ctypes releases the GIL during the
    engine's calls, so the ranks' collectives rendezvous); returns the results in rank order
    and re-raises the first exception."""
    import threading
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001 -- re-raised below
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return out


def checkpoint_info(path):
    """Host-only look at a checkpoint file: dict of version, n_layers, num_nodes, input_dim,
    output_dim, adam_steps, epochs, weights.  PgcnError(PGCN_E_IO) for an invalid file."""
    info = (c_ll * 8)()
    check(lib.pgcn_checkpoint_info(os.fsencode(path), info), f"checkpoint_info {path}")
    keys = ("version", "n_layers", "num_nodes", "input_dim", "output_dim", "adam_steps", "epochs",
            "weights")
    return dict(zip(keys, (int(x) for x in info)))


CKPT_RESIDUAL = 1
CKPT_LAYERNORM = 2  # version-2 files: the scale / shift tensor behind the layer weights
CKPT_MULTILABEL = 4  # saved by a multi-label engine (no payload change)
CKPT_ATTENTION = 8  # version-4 files: the attention tensor last in the payloads
CKPT_SAGE = 16  # version-6 files: a GraphSAGE engine's, with the {aggregator, root_weight} block
CKPT_READOUT = 32  # version-7 files: a graph-classification engine's, with its three blocks
CKPT_LINKS = 64  # version-8 files: a link-prediction engine's, with its four blocks


def checkpoint_flags(path):
    """Host-only: a checkpoint file's header flags (bit 0, CKPT_RESIDUAL: saved by an engine with
    residual layers; bit 1, CKPT_LAYERNORM: by one with LayerNorm; bit 2, CKPT_MULTILABEL: by a
    multi-label one; bit 3, CKPT_ATTENTION: by an attention one).  PgcnError(PGCN_E_IO) for an
    invalid file or unknown flag bits."""
    st = lib.pgcn_checkpoint_flags(os.fsencode(path))
    check(min(st, 0), f"checkpoint_flags {path}")
    return st


def checkpoint_attention(path):
    """Host-only: (heads, attention dropout) of the engine that saved the file -- a version-5
    file's extension; (1, 0.0) for versions 1-4.  PgcnError(PGCN_E_IO) for an invalid file."""
    heads, p = c_int(), c_float()
    check(lib.pgcn_checkpoint_attention(os.fsencode(path), ctypes.byref(heads), ctypes.byref(p)),
          f"checkpoint_attention {path}")
    return heads.value, p.value


def checkpoint_sage(path):
    """Host-only: (aggregator, root_weight) of the engine that saved the file -- a version-6
    file's block; (0, 0) for versions 1-5.  PgcnError(PGCN_E_IO) for an invalid file."""
    agg, root = c_int(), c_int()
    check(lib.pgcn_checkpoint_sage(os.fsencode(path), ctypes.byref(agg), ctypes.byref(root)),
          f"checkpoint_sage {path}")
    return agg.value, root.value


def checkpoint_links(path):
    """Host-only: (link decoder, num_pairs) of the engine that saved the file -- a version-8
    file's block; (0, 0) for versions 1-7.  PgcnError(PGCN_E_IO) for an invalid file."""
    dec, e = c_int(), c_ll()
    check(lib.pgcn_checkpoint_links(os.fsencode(path), ctypes.byref(dec), ctypes.byref(e)),
          f"checkpoint_links {path}")
    return dec.value, e.value


def checkpoint_readout(path):
    """Host-only: (readout mode, num_graphs) of the engine that saved the file -- a version-7
    file's block; (0, 0) for versions 1-6.  PgcnError(PGCN_E_IO) for an invalid file."""
    mode, g = c_int(), c_int()
    check(lib.pgcn_checkpoint_readout(os.fsencode(path), ctypes.byref(mode), ctypes.byref(g)),
          f"checkpoint_readout {path}")
    return mode.value, g.value


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    check(lib.pgcn_comm_unique_id(buf), "comm_unique_id")
    return buf.raw


# --------------------------------------------------------------------------- host helpers
def rng_seed(seed=0):
    s = (c_u64 * 2)()
    if seed:
        lib.pgcn_rng_seed_glibc(seed, s)
    else:
        lib.pgcn_rng_seed(s)
    return np.array([s[0], s[1]], np.uint64)


def rng_jump(state, k):
    s = (c_u64 * 2)(int(state[0]), int(state[1]))
    lib.pgcn_rng_jump(s, int(k))
    return np.array([s[0], s[1]], np.uint64)


def rng_jump_table(period):
    t = np.zeros(16 * 256 * 2, np.uint64)
    check(lib.pgcn_rng_jump_table(int(period), _ptr(t)), "rng_jump_table")
    return t


def partition_bounds(indptr, world):
    indptr = np.ascontiguousarray(indptr, np.int32)
    b = np.zeros(world + 1, np.int32)
    mr = c_int()
    check(lib.pgcn_partition_bounds(len(indptr) - 1, _ptr(indptr), world, _ptr(b),
                                    ctypes.byref(mr)), "partition_bounds")
    return b, mr.value


def partition_subgraph(indptr, indices, world, rank):
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    n = len(indptr) - 1
    _, maxrows = partition_bounds(indptr, world)
    nnz = lib.pgcn_partition_subgraph(n, _ptr(indptr), _ptr(indices), world, rank, None, None, None)
    if nnz < 0:
        raise PgcnError(int(nnz), "partition_subgraph")
    sp = np.zeros(world * maxrows + 1, np.int32)
    si = np.zeros(max(nnz, 1), np.int32)
    sv = np.zeros(max(nnz, 1), np.float32)
    lib.pgcn_partition_subgraph(n, _ptr(indptr), _ptr(indices), world, rank, _ptr(sp), _ptr(si),
                                _ptr(sv))
    return sp, si[:nnz], sv[:nnz]


def csr_transpose(indptr, indices, n_cols):
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    m, nnz = len(indptr) - 1, int(indptr[-1])
    cp = np.zeros(n_cols + 1, np.int32)
    cr = np.zeros(max(nnz, 1), np.int32)
    cpos = np.zeros(max(nnz, 1), np.int32)
    check(lib.pgcn_csr_transpose(m, n_cols, _ptr(indptr), _ptr(indices), _ptr(cp), _ptr(cr),
                                 _ptr(cpos)), "csr_transpose")
    return cp, cr[:nnz], cpos[:nnz]


EXPORTED = [
    "pgcn_status_string", "pgcn_version", "pgcn_rng_seed", "pgcn_rng_seed_glibc", "pgcn_rng_jump",
    "pgcn_graph_create", "pgcn_graph_create_values", "pgcn_debug_rank_graph",
    "pgcn_graph_destroy", "pgcn_graph_nnz", "pgcn_graphsum", "pgcn_gemm", "pgcn_gemm_tn_workspace",
    "pgcn_gemm_tn", "pgcn_mask_nibbles", "pgcn_gemm_xstream", "pgcn_gemm_xstream_dual",
    "pgcn_gemm_tn_xstream", "pgcn_gemm_xstream_flat", "pgcn_gemm_tn_xstream_flat",
    "pgcn_spmm_csr", "pgcn_spmm_csc_bwd", "pgcn_csr_transpose",
    "pgcn_rng_jump_table", "pgcn_dropout_mask", "pgcn_dropout_apply", "pgcn_relu_fwd",
    "pgcn_relu_bwd", "pgcn_residual_fwd", "pgcn_residual_bwd", "pgcn_params_sizeof",
    "pgcn_layernorm_fwd", "pgcn_layernorm_bwd_workspace", "pgcn_layernorm_bwd",
    "pgcn_debug_layernorm_fwd_tail",
    "pgcn_gat_scores", "pgcn_gat_fwd", "pgcn_gat_bwd_workspace", "pgcn_gat_bwd",
    "pgcn_gat_scores_mh", "pgcn_gat_fwd_mh", "pgcn_gat_bwd_workspace_mh", "pgcn_gat_bwd_mh",
    "pgcn_graph_create_mean", "pgcn_agg_max_fwd", "pgcn_agg_max_bwd",
    "pgcn_checkpoint_flags", "pgcn_checkpoint_attention", "pgcn_checkpoint_sage", "pgcn_xent_blocks", "pgcn_xent_fwd", "pgcn_finalize", "pgcn_adam",
    "pgcn_adam_step_size", "pgcn_params_default", "pgcn_gcn_create", "pgcn_comm_unique_id",
    "pgcn_gcn_create_dist", "pgcn_gcn_create_peer", "pgcn_loopback_create",
    "pgcn_loopback_destroy",
    "pgcn_debug_gcn_create_solo",
    "pgcn_gcn_create_loopback", "pgcn_gcn_query", "pgcn_gcn_destroy", "pgcn_gcn_train_epoch", "pgcn_gcn_eval",
    "pgcn_gcn_epoch_async", "pgcn_gcn_sync", "pgcn_gcn_results", "pgcn_gcn_run",
    "pgcn_gcn_get_var", "pgcn_gcn_num_vars", "pgcn_gcn_profile", "pgcn_gcn_profile_read",
    "pgcn_gcn_set_var", "pgcn_gcn_save", "pgcn_gcn_load", "pgcn_checkpoint_info",
    "pgcn_gcn_predict", "pgcn_gcn_confusion", "pgcn_predict_rows", "pgcn_confusion",
    "pgcn_gcn_profile_read_mm",
    "pgcn_gcn_node_range", "pgcn_dataset_load", "pgcn_dataset_load_cached", "pgcn_dataset_save",
    "pgcn_dataset_load_binary", "pgcn_dataset_binarize", "pgcn_dataset_synthetic",
    "pgcn_dataset_view",
    "pgcn_dataset_free", "pgcn_partition_bounds", "pgcn_partition_subgraph", "pgcn_debug_set",
    "pgcn_debug_knob",
    "pgcn_debug_lds_check", "pgcn_debug_lds_counts", "pgcn_debug_path_count",
    "pgcn_debug_empty_launches", "pgcn_debug_exp_check", "pgcn_debug_div_check",
    "pgcn_debug_ring_slice_rows", "pgcn_debug_xent_fwd", "pgcn_debug_out_xent",
    "pgcn_debug_finalize_ring", "pgcn_debug_tn_reduce_blocks_workspace",
    "pgcn_debug_tn_reduce_blocks", "pgcn_debug_tn_reduce_one_pass",
    "pgcn_debug_gemm_nib", "pgcn_debug_gemm_tn_nib",
    "pgcn_debug_spmm_csr", "pgcn_debug_spmm_csc_bwd", "pgcn_debug_dropout_mask",
    "pgcn_debug_dropout_mask2", "pgcn_debug_dropout_apply",
    "pgcn_bce_fwd", "pgcn_predict_multilabel_rows", "pgcn_multilabel_counts",
    "pgcn_gcn_predict_multilabel", "pgcn_gcn_multilabel_counts", "pgcn_dataset_set_multilabel",
    "pgcn_dataset_load_labels",
    "pgcn_readout_chunk_rows", "pgcn_readout_workspace", "pgcn_readout_fwd", "pgcn_readout_bwd",
    "pgcn_dataset_set_graphs", "pgcn_dataset_load_graphs", "pgcn_checkpoint_readout",
    "pgcn_links_create", "pgcn_links_destroy", "pgcn_link_segment_slots", "pgcn_links_slots",
    "pgcn_link_score_fwd", "pgcn_link_score_bwd", "pgcn_debug_links_incidence",
    "pgcn_checkpoint_links", "pgcn_gcn_predict_links", "pgcn_gcn_link_counts",
    "pgcn_gcn_score_pairs", "pgcn_dataset_set_links", "pgcn_dataset_load_links",
    "pgcn_rank_queries_create", "pgcn_rank_queries_destroy", "pgcn_link_rank_tile",
    "pgcn_link_rank_scores", "pgcn_link_rank", "pgcn_debug_rank_filter", "pgcn_gcn_link_ranks",
    "pgcn_topk_queries_create", "pgcn_topk_queries_destroy", "pgcn_topk_queries_workspace",
    "pgcn_link_topk_tile", "pgcn_link_topk_splits", "pgcn_link_topk_chunk", "pgcn_link_topk",
    "pgcn_debug_topk_filter", "pgcn_gcn_top_links",
]
