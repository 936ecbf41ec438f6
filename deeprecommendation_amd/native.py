"""ctypes binding of libncf_hip.so (include/ncf_abi.h) + thin torch-tensor marshalling.

PyTorch is used for device memory and streams only: every function here takes CUDA(=HIP) tensors, passes raw
device pointers + sizes + the current HIP stream to the C ABI and returns tensors it allocated for the result.
There is NO fallback: if the shared library is missing or a tensor is not on a GPU, these functions raise.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NCF_HIP_LIBRARY") or os.path.join(_HERE, "libncf_hip.so")   # the override is for A/B builds (tools/ab_build.sh)

NCF_F32, NCF_BF16 = 0, 1
NCF_OK, NCF_EINVAL, NCF_EUNSUPPORTED, NCF_ELAUNCH, NCF_EWORKSPACE = 0, -1, -2, -3, -4
ATT_MLP, ATT_LINEAR, ATT_COS, ATT_MLP_SCALED = 0, 1, 2, 3
ATT_SCALE_LOG2 = 64   # include/ncf_abi.h NCF_ATT_SCALE_LOG2

_c_i64 = ctypes.c_int64
_c_p = ctypes.c_void_p
_c_int = ctypes.c_int
_c_size = ctypes.c_size_t

# name -> (restype, argtypes); the parity tests check that every symbol declared in include/ncf_abi.h is here
# and exported by the library.
SIGNATURES = {
    "ncf_version": (_c_int, []),
    "ncf_last_error": (ctypes.c_char_p, []),
    "ncf_build_arch": (ctypes.c_char_p, []),
    "ncf_build_id": (ctypes.c_char_p, []),
    "ncf_probe_mfma_bf16": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p]),
    "ncf_probe_copy": (_c_int, [_c_p, _c_p, _c_i64, _c_p]),
    "ncf_probe_gather_read": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_p]),
    "ncf_set_option": (_c_int, [ctypes.c_char_p, _c_int]),
    "ncf_get_option": (_c_int, [ctypes.c_char_p, _c_p]),
    "ncf_bucket_ids": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_bucket_dedup_table_slots": (_c_size, [_c_i64]),
    "ncf_bucket_ids_dedup": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_gather_buckets": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_int, _c_i64, _c_int, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_gather_concat": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_int,
                                   _c_p, _c_i64, _c_p, _c_p]),
    "ncf_gather_dot": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p]),
    "ncf_mlp_workspace_bytes": (_c_size, [_c_int, _c_i64, _c_int, _c_p]),
    "ncf_mlp_forward": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_i64, _c_p]),
    "ncf_score_fused_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_p]),
    "ncf_mlp_packed_bytes": (_c_size, [_c_int, _c_int, _c_p]),
    "ncf_mlp_pack": (_c_int, [_c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p]),
    "ncf_score_fused": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_int,
                                 _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_spmm_csr": (_c_int, [_c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p,
                              _c_i64, _c_p, _c_int, _c_p]),
    "ncf_spmm_csr_dropout": (_c_int, [_c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p,
                                      _c_i64, _c_p, _c_int, _c_p, ctypes.c_uint32, ctypes.c_float, _c_p]),
    "ncf_degree_accumulate": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_edge_coef": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p]),
    "ncf_edge_keep": (_c_int, [_c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p, ctypes.c_float, ctypes.c_uint32, _c_p,
                               _c_p, _c_p, _c_p]),
    "ncf_scale_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, ctypes.c_float, _c_p, _c_i64, _c_p]),
    "ncf_attn_forward": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_p, _c_p,
                                  _c_i64, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_attn_forward_dropout": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_p, _c_p,
                                          _c_i64, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_i64, _c_p, ctypes.c_uint32, ctypes.c_float, _c_p]),
    "ncf_attn_backward": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_int,
                                   _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_p, ctypes.c_uint32, ctypes.c_float, _c_p]),
    "ncf_attn_forward_train": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_p, _c_p,
                                        _c_i64, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_i64, _c_p, ctypes.c_uint32, ctypes.c_float,
                                        ctypes.c_uint32, ctypes.c_float, _c_p]),
    "ncf_attn_backward_train": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_int,
                                         _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_p, ctypes.c_uint32, ctypes.c_float,
                                         ctypes.c_float, _c_p]),
    "ncf_attn_forward_grouped": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_p, _c_p,
                                          _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_i64, _c_int, _c_p, _c_p,
                                          _c_i64, _c_p, _c_p, _c_p]),
    "ncf_attn_grouped_plan": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _c_int, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_group_pairs_workspace_bytes": (_c_size, [_c_i64]),
    "ncf_group_pairs": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_group_pairs_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_dense_csr_workspace_bytes": (_c_size, [_c_i64]),
    "ncf_dense_csr_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_size, _c_p]),
    "ncf_dense_csr_fill": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_pair_rows_count": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_pair_rows_fill": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int,
                                    ctypes.c_float, ctypes.c_float, _c_p, _c_p]),
    "ncf_attn_candidates_supported": (_c_int, [_c_int, _c_int, _c_int]),
    "ncf_attn_candidates_workspace_bytes": (_c_size, [_c_i64]),
    "ncf_attn_candidates": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p, _c_int, _c_p, _c_p, _c_int, _c_p, _c_i64, _c_p, _c_i64,
                                     _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_attn_candidates_pack_floats": (_c_size, [_c_int, _c_int]),
    "ncf_attn_candidates_packed_workspace_bytes": (_c_size, [_c_i64, _c_int, _c_i64]),
    "ncf_attn_candidates_pack": (_c_int, [_c_p, _c_i64, _c_int, _c_int, _c_p, _c_p]),
    "ncf_attn_candidates_packed": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_int, _c_p, _c_p, _c_int, _c_p, _c_i64, _c_p, _c_i64,
                                            _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_attn_split_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int]),
    "ncf_attn_split_workspace_bytes": (_c_size, [_c_i64, _c_int, _c_int]),
    "ncf_attn_forward_split": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_p, _c_p,
                                        _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_i64, _c_int, _c_p, _c_p,
                                        _c_i64, _c_int, _c_int, _c_p, _c_size, _c_p]),
    "ncf_attn_tail_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int]),
    "ncf_attn_tail_pack_weight": (_c_int, [_c_p, _c_int, _c_int, _c_p, _c_p]),
    "ncf_attn_tail": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_int, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_int,
                               _c_p, ctypes.c_float, _c_int, _c_p, _c_i64, _c_p]),
    "ncf_attn_logits": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p, ctypes.c_float, _c_p, _c_i64, _c_p]),
    "ncf_attn_cross_supported": (_c_int, [_c_int]),
    "ncf_attn_cross_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p]),
    "ncf_attn_cross": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_int,
                                _c_p, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_attn_explain_max_reasons": (_c_int, []),
    "ncf_attn_explain": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_int,
                                  _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_attn_stats_workspace_bytes": (_c_size, [_c_i64]),
    "ncf_attn_stats": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64,
                                _c_p, _c_p, _c_size, _c_p]),
    "ncf_edge_softmax_csr": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p]),
    "ncf_edge_softmax_segmented_workspace_bytes": (_c_size, [_c_i64, _c_i64]),
    "ncf_edge_softmax_segmented": (_c_int, [_c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_size, _c_p]),
    "ncf_gat_edge_softmax_workspace_bytes": (_c_size, [_c_i64, _c_i64]),
    "ncf_gat_edge_softmax": (_c_int, [_c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_size, _c_p]),
    "ncf_gat_edge_grad_workspace_bytes": (_c_size, [_c_i64, _c_i64]),
    "ncf_gat_edge_grad": (_c_int, [_c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int,
                                   ctypes.c_float, ctypes.c_uint32, _c_p, _c_p, _c_size, _c_p]),
    "ncf_gat_source_reduce": (_c_int, [_c_p, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_score_fused_partial_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_p]),
    "ncf_score_fused_partial_in_lds": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_p]),
    "ncf_layer1_partial": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p]),
    "ncf_score_fused_partial": (_c_int, [_c_int, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64,
                                         _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_score_folded_supported": (_c_int, [_c_int, _c_int, _c_int]),
    "ncf_score_folded": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p,
                                  _c_p, _c_p, _c_p]),
    "ncf_linear_forward": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_i64, _c_p]),
    "ncf_linear_plan": (_c_int, [_c_i64, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_gemm_tn_workspace_bytes": (_c_size, [_c_i64, _c_int, _c_int]),
    "ncf_gemm_tn": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_int, _c_p, _c_i64, _c_p, _c_size, _c_p]),
    "ncf_colsum_workspace_bytes": (_c_size, [_c_i64, _c_int]),
    "ncf_colsum": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_size, _c_p]),
    "ncf_relu_backward": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p]),
    "ncf_relu_backward_out": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int, ctypes.c_float, _c_p]),
    "ncf_scatter_add_rows": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_i64, _c_i64, _c_p, _c_p]),
    "ncf_l2_normalize_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p]),
    "ncf_user_profiles": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_kmf_epoch": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_int,
                               ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_int, _c_p, _c_p, _c_p]),
    "ncf_kmf_fold_users": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64,
                                    ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_int, _c_p, _c_p, _c_p]),
    "ncf_knn_item_sq": (_c_int, [_c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_knn_sim_rows": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int,
                                  ctypes.c_float, _c_int, _c_p, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_knn_scores": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_i64, _c_i64, _c_int,
                                ctypes.c_float, _c_int, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_knn_predict": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_int,
                                 ctypes.c_float, _c_p, _c_p, _c_p]),
    "ncf_als_gram_workspace_bytes": (_c_size, [_c_i64, _c_int]),
    "ncf_als_gram": (_c_int, [_c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_size, _c_p]),
    "ncf_als_solve_rows": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_p, ctypes.c_float,
                                    ctypes.c_float, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_ease_gram": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_p,
                               _c_p]),
    "ncf_ease_invert_workspace_bytes": (_c_size, [_c_i64]),
    "ncf_ease_invert": (_c_int, [_c_p, _c_i64, _c_i64, ctypes.c_float, _c_p, _c_size, _c_p, _c_p]),
    "ncf_ease_weights": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_p]),
    "ncf_ease_scores": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_p, _c_i64,
                                 _c_p, _c_p]),
    "ncf_ease_predict": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_slim_solve": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, ctypes.c_float, ctypes.c_float, _c_int, _c_int, _c_int, ctypes.c_float,
                                _c_p, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_mmr_supported": (_c_int, [_c_int, _c_int, _c_int]),
    "ncf_mmr_rerank": (_c_int, [_c_p, _c_i64, _c_int, _c_i64, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_int, ctypes.c_float, _c_int, _c_p, _c_p,
                                _c_p, _c_p, _c_p]),
    "ncf_gather_cols": (_c_int, [_c_p, _c_i64, _c_p, _c_p, _c_i64, _c_int, _c_i64, _c_p, _c_i64, _c_p, _c_p]),
    "ncf_scatter_add_cols": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_i64, _c_i64, _c_p, _c_p]),
    "ncf_topk_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int]),
    "ncf_topk_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p]),
    "ncf_dot_topk_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_int]),
    "ncf_dot_topk": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_int, _c_p,
                              _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_mlp_topk_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_p, _c_int]),
    "ncf_mlp_topk_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_int, _c_p, _c_int]),
    "ncf_mlp_topk": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_i64,
                              _c_int, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_rank_max_targets": (_c_int, []),
    "ncf_rank_rows_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_i64]),
    "ncf_rank_rows": (_c_int, [_c_p, _c_i64, _c_i64, _c_i64, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_p, _c_size, _c_p]),
    "ncf_dot_rank_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_i64, _c_int]),
    "ncf_dot_rank": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p,
                              _c_i64, _c_int, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p, _c_p]),
    "ncf_mlp_rank_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_p, _c_int]),
    "ncf_mlp_rank_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_int, _c_p, _c_i64, _c_int]),
    "ncf_mlp_rank": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_p, _c_p, _c_i64, _c_i64,
                              _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_size, _c_p, _c_p, _c_p]),
    "ncf_ranking_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p]),
    "ncf_neumf_supported": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ncf_neumf_score": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_p, _c_p, _c_i64, _c_int,
                                 _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ncf_neumf_topk_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_p, _c_int, _c_int]),
    "ncf_neumf_topk": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_int, _c_int,
                                _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_size,
                                _c_p, _c_p]),
    "ncf_neumf_rank_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_p, _c_int, _c_i64, _c_int]),
    "ncf_neumf_rank": (_c_int, [_c_int, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_p, _c_i64, _c_int, _c_int, _c_int,
                                _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p,
                                _c_p, _c_size, _c_p, _c_p, _c_p]),
    "ncf_dot_softmax_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p]),
    "ncf_dot_lse_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int]),
    "ncf_dot_lse": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_i64, _c_int, ctypes.c_float, _c_p, _c_p,
                             _c_p, _c_size, _c_p, _c_p]),
    "ncf_dot_softmax_grad_workspace_bytes": (_c_size, [_c_i64, _c_i64, _c_int, _c_int]),
    "ncf_dot_softmax_grad": (_c_int, [_c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_i64, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_p,
                                      ctypes.c_float, _c_int, _c_p, _c_p, _c_size, _c_p, _c_p]),
    "ncf_adam_step": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                               ctypes.c_float, _c_i64, _c_p]),
    "ncf_adam_rows": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_i64, _c_int, _c_p, _c_p, _c_i64, _c_p, _c_i64, ctypes.c_float, ctypes.c_float,
                               ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_i64, _c_p, _c_p]),
    "ncf_negative_cdf": (_c_int, [_c_p, _c_i64, _c_p, ctypes.c_float, _c_p, _c_p, _c_p]),
    "ncf_sample_negatives": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_p, _c_i64, ctypes.c_uint32, _c_i64, _c_p, _c_p, _c_p]),
    "ncf_sample_unseen": (_c_int, [_c_p, _c_p, _c_i64, _c_i64, _c_p, _c_i64, _c_int, ctypes.c_uint32, _c_i64, _c_p, _c_p, _c_p]),
}

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libncf_hip: {msg} (status {code})")
        self.code = code


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the HIP library and bind every ABI symbol.  Raises if it is absent — there is no CPU path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(needs hipcc). deeprecommendation_amd has no CPU fallback.")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if path is None:
        if not os.environ.get("NCF_HIP_LIBRARY"):        # an A/B build named by the override is loaded as it is
            _check_build_id(lib, p)
        _lib = lib
        _options_from_environment(lib)
    return lib


def _check_build_id(lib, path):
    """A library built from other sources than the ones next to it is refused (mtime said nothing about a checkout or a copy)."""
    try:
        from .csrc import build as _build
        want = _build.source_id()
    except (ImportError, OSError):        # sources not shipped: nothing to compare with
        return
    have = lib.ncf_build_id().decode()
    if have != want:
        raise RuntimeError(f"{path} is stale: built from sources {have}, the sources here are {want}. "
                           "Rebuild: python -m deeprecommendation_amd.csrc.build")


# ncf_set_option values by name (include/ncf_abi.h); 0 / "auto" = choose by shape
OPTION_VALUES = {
    "bf16_kernel": {"auto": 0, "ws": 1, "stream": 2, "ws8": 3},
    "linear_kernel": {"auto": 0, "rs": 1, "rsp": 2},
    "linear_kslices": {"auto": 0, "4": 4, "8": 8},
    "attn_grouped_kernel": {"auto": 0, "lds": 1, "scalar": 2},
    "gather_kernel": {"auto": 0, "step": 1, "persistent": 2},
}
_ENV_OPTIONS = {"NCF_BF16_KERNEL": "bf16_kernel", "NCF_LINEAR_KERNEL": "linear_kernel", "NCF_LINEAR_KS": "linear_kslices",
                "NCF_ATTN_GROUPED_KERNEL": "attn_grouped_kernel", "NCF_GATHER_KERNEL": "gather_kernel"}


def set_option(name: str, value) -> None:
    """Kernel-selection override (A/B tools, tests that drive every variant).  ``value``: the symbolic name
    ("ws", "rsp", …, "auto") or the integer of include/ncf_abi.h.  Process-wide; "auto" / 0 restores the default."""
    lib = load_library()
    if isinstance(value, str):
        try:
            value = OPTION_VALUES[name][value]
        except KeyError:
            raise ValueError(f"option {name!r} has no value {value!r}") from None
    _check(lib.ncf_set_option(name.encode(), int(value)))


def _query(fn, ins, outs):
    """A host-only query of the library: calls ``fn(*ins, &cell, ...)`` with one zeroed cell per ctypes type of ``outs``, in order,
    under _check, and returns the cells' values as a tuple."""
    cells = [t() for t in outs]
    _check(fn(*ins, *map(ctypes.byref, cells)))
    return tuple([c.value for c in cells])


def get_option(name: str) -> int:
    return _query(load_library().ncf_get_option, (name.encode(),), (_c_int,))[0]


def _options_from_environment(lib) -> None:
    """The library never reads the environment; the dev tools' NCF_* variables are applied HERE, once, at load."""
    for var, name in _ENV_OPTIONS.items():
        v = os.environ.get(var)
        if v:
            if v not in OPTION_VALUES[name]:
                raise ValueError(f"{var}={v!r}: expected one of {sorted(OPTION_VALUES[name])}")
            rc = lib.ncf_set_option(name.encode(), OPTION_VALUES[name][v])
            if rc != NCF_OK:
                raise NativeError(rc, lib.ncf_last_error().decode())


def _check(rc: int):
    if rc != NCF_OK:
        raise NativeError(rc, load_library().ncf_last_error().decode())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def host_seed() -> int:
    """A 31-bit seed for the library's counter-based draws (dropout masks, the keep rule, the samplers) from torch's default HOST
    generator: one draw per call, no device synchronisation, and torch.manual_seed makes a run repeat."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def _stream(t: torch.Tensor) -> int:
    """torch's current stream on t's device as a raw hipStream_t (every launch of the library goes there).  The raw accessor costs
    0.3 us where torch.cuda.current_stream() builds a Stream object (2.3 us, five times per AttentionNCF forward)."""
    if _raw_stream is not None:
        idx = t.device.index
        return _raw_stream(idx if idx is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU (got {t.device}); deeprecommendation_amd has no CPU path")


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return NCF_F32
    if t.dtype == torch.bfloat16:
        return NCF_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _rows2d(t: torch.Tensor, what: str):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what} must be 2-D with unit inner stride")
    return t.shape[0], t.shape[1], t.stride(0)


def _idx(t: Optional[torch.Tensor], B: Optional[int] = None):
    if t is None:
        return None
    if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
        raise ValueError("index tensors must be contiguous 1-D int64")
    return t


# ------------------------------------------------------------------ the argument checks of the "who: ..." wrappers
# Each raises ValueError("<who>: <argument> ...") naming the limit that was broken, and touches no device: a wrapper runs all of
# them, then _dev_all, and only then loads the library and allocates.
def _dev_all(*pairs):
    """The device sweep: every ``(tensor, name)`` pair given must live on the GPU; a None tensor is skipped."""
    for t, what in pairs:
        if t is not None:
            _dev(t, what)


def _int_in(who, v, what, lo, hi):
    """``v`` as an int in lo .. hi; a bool or a float is refused, a numpy integer taken."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
        raise ValueError(f"{who}: {what} = {v!r} (an integer in {lo} .. {hi})")
    return int(v)


def _finite(who, v, what, lo=None):
    """``v`` as a finite float (>= ``lo`` when given); a bool is refused, a numpy scalar taken."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or (lo is not None and v < lo):
        raise ValueError(f"{who}: {what} = {v!r} is not a finite number" + ("" if lo is None else f" >= {lo}"))
    return float(v)


def _vec1d(who, t, what, dt, n=None):
    if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous 1-D {dt} tensor")
    if n is not None and t.numel() != n:
        raise ValueError(f"{who}: {what} has {t.numel()} entries, expected {n}")


def _out1d(who, t, what, dt, n):
    if t is not None and (not torch.is_tensor(t) or t.dtype != dt or not t.is_contiguous() or t.numel() != n):
        raise ValueError(f"{who}: {what} must be a contiguous {dt} tensor of {n} entries")


def _csr(who, ptr, idx, val, names, rows=None):
    """Checks one CSR (pointers int64, ids int32, values fp32, contiguous 1-D); returns (rows, nnz)."""
    _vec1d(who, ptr, names[0], torch.int64, None if rows is None else rows + 1)
    if ptr.numel() < 1:
        raise ValueError(f"{who}: {names[0]} is empty")
    _vec1d(who, idx, names[1], torch.int32)
    _vec1d(who, val, names[2], torch.float32, idx.numel())
    return ptr.numel() - 1, idx.numel()


def _table_f32(who, t, what, min_cols=1):
    """A 2-D float32 table of at least ``min_cols`` columns whose inner stride is 1 (any, when it is one column wide)."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{who}: {what} must be a 2-D float32 tensor with unit inner stride")
    if t.shape[1] < min_cols:
        raise ValueError(f"{who}: {what} has rows of {t.shape[1]} floats, fewer than the {min_cols} needed")


def _out2d(who, out, rows, cols, like, swept, contiguous=False, wider=False):
    """The optional float32 ``out`` of a wrapper, and the end of its checks: a given ``out`` must be (rows, cols) — (rows, >= cols)
    with ``wider`` — with unit inner stride and any row stride, or ``contiguous``; then the device sweep over ``swept`` and ``out``;
    only after both is an absent ``out`` allocated beside ``like``.  Returns the tensor to write."""
    if out is not None:
        ok = torch.is_tensor(out) and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == rows
        ok = ok and (out.shape[1] >= cols if wider else out.shape[1] == cols)
        if not (ok and (out.is_contiguous() if contiguous else out.shape[1] <= 1 or out.stride(1) == 1)):
            raise ValueError(f"{who}: out must be a ({rows}, {'>= ' if wider else ''}{cols}) float32 tensor, "
                             + ("contiguous" if contiguous else "with unit inner stride"))
    _dev_all(*swept, (out, "out"))
    return torch.empty((rows, cols), dtype=torch.float32, device=like.device) if out is None else out


def _workspace(nbytes, device) -> torch.Tensor:
    """The scratch of one call: ``nbytes`` as the entry's *_workspace_bytes said, and never an empty tensor (whose pointer is null).
    The C call is told ``nbytes``, not the padded size."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


_flags = {}


def _flag(kind, device) -> torch.Tensor:
    """The sticky int32 flag word of ``kind`` on ``device``: one zeroed tensor per (kind, device), which kernels set and a
    ``check_*`` reads and clears."""
    f = _flags.get((kind, device))
    if f is None:
        f = _flags[kind, device] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


# the bits of the flag words with several meanings (include/ncf_abi.h NCF_<name>; tests/test_abi_symbols.py compares them)
KMF_FLAG_ID, KMF_FLAG_BLOCK, KMF_FLAG_PTR = 1, 2, 4
ALS_FLAG_COL, ALS_FLAG_PTR, ALS_FLAG_ORDER, ALS_FLAG_VAL, ALS_FLAG_PIVOT = 1, 2, 4, 8, 16
EASE_FLAG_ORDER, EASE_FLAG_PIVOT = 1, 2
UNSEEN_FLAG_PICK, UNSEEN_FLAG_FEW = 1, 256

# kind -> (prefix of the message or None, [(bit, what a kernel met, what check_* raises for it)], whether the message ends in the
# word's value).  A word with one meaning whatever its value has the one row of bit ~0.
_FLAG_WORDS = {
    "oob": (None, [(~0, "index out of range in an embedding gather", IndexError)], False),
    "pair_rows": (None, [(~0, "a pair's rated entries did not fit the capacity pair_rows was given (max_row_len too small)",
                          OverflowError)], False),
    "rank_overflow": (None, [(~0, "a row has more targets than the max_targets the rank call was given", OverflowError)], False),
    "kmf": ("KernelMF", [(KMF_FLAG_ID, "an id outside its table", IndexError),
                         (KMF_FLAG_BLOCK, "a sample filed in the wrong block", IndexError),
                         (KMF_FLAG_PTR, "a block / row pointer outside the samples", IndexError)], True),
    "knn": ("ItemKNN", [(~0, "a row of the ratings CSR does not hold strictly ascending columns", ValueError)], False),
    "als": ("ImplicitALS", [(ALS_FLAG_COL, "a column outside the fixed table", IndexError),
                            (ALS_FLAG_PTR, "a row or a row pointer outside the ratings", IndexError),
                            (ALS_FLAG_ORDER, "a row whose columns do not strictly ascend", ValueError),
                            (ALS_FLAG_VAL, "a value that is negative or not finite", ValueError),
                            (ALS_FLAG_PIVOT, "a pivot that is not positive and finite", ValueError)], True),
    "ease": ("EASE", [(EASE_FLAG_ORDER, "a row of the ratings CSR does not hold strictly ascending columns", ValueError),
                      (EASE_FLAG_PIVOT, "a pivot of the inversion that is not positive and finite", ValueError)], True),
    "unseen": ("sample_unseen", [(UNSEEN_FLAG_PICK, "a pick outside the users", IndexError),
                                 (UNSEEN_FLAG_FEW, "a user has fewer unseen items than the draws asked for", ValueError)], True),
}


def _check_flag(kind, device, flag=None):
    """Synchronising check of ``kind``'s flag word on ``device`` (``flag``: another word): when it is not zero, clears it and raises
    with the text of every set bit and, where _FLAG_WORDS says so, its value — IndexError when an id or a pointer was at fault, else
    the type of the word's last row."""
    f = _flag(kind, device) if flag is None else flag
    bits = int(f.item())
    if bits:
        f.zero_()
        prefix, rows, numbered = _FLAG_WORDS[kind]
        hit = [(text, exc) for bit, text, exc in rows if bits & bit]
        exc = IndexError if any(e is IndexError for _, e in hit) else rows[-1][2]
        raise exc((f"{prefix}: " if prefix else "") + ", ".join(text for text, _ in hit) + (f" (flag {bits})" if numbered else ""))


def _oob_flag(device) -> torch.Tensor:
    return _flag("oob", device)


def check_oob(device):
    """Synchronising check of the sticky out-of-range flag (torch indexing raises IndexError in the reference)."""
    _check_flag("oob", device)


# ------------------------------------------------------------------ K1
def gather_concat(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: Optional[torch.Tensor] = None,
                  idxB: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, B: Optional[int] = None):
    lib = load_library()
    _dev(tabA, "tabA")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    rowsB = EB = ldB = 0
    if tabB is not None:
        _dev(tabB, "tabB")
        rowsB, EB, ldB = _rows2d(tabB, "tabB")
        if tabB.dtype != tabA.dtype:
            raise TypeError("tables must share a dtype")
    idxA, idxB = _idx(idxA), _idx(idxB)
    if B is None:
        B = idxA.numel() if idxA is not None else (idxB.numel() if idxB is not None else rowsA)
    if out is None:
        out = torch.empty((B, EA + EB), dtype=tabA.dtype, device=tabA.device)
    _, _, ldo = _rows2d(out, "out")
    _check(lib.ncf_gather_concat(_dt(tabA), _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(idxA), _ptr(idxB), B, EA, EB,
                                 _ptr(out), ldo, _ptr(_oob_flag(tabA.device)), _stream(tabA)))
    return out


def gather_dot(tabA: torch.Tensor, idxA, tabB: torch.Tensor, idxB, B: Optional[int] = None):
    lib = load_library()
    _dev(tabA, "tabA"), _dev(tabB, "tabB")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    rowsB, EB, ldB = _rows2d(tabB, "tabB")
    if EA != EB or tabA.dtype != tabB.dtype:
        raise ValueError("gather_dot needs equal widths and dtypes")
    idxA, idxB = _idx(idxA), _idx(idxB)
    if B is None:
        B = idxA.numel() if idxA is not None else idxB.numel()
    out = torch.empty((B, 1), dtype=torch.float32, device=tabA.device)
    _check(lib.ncf_gather_dot(_dt(tabA), _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(idxA), _ptr(idxB), B, EA,
                              _ptr(out), _ptr(_oob_flag(tabA.device)), _stream(tabA)))
    return out


def bucket_ids(idx: torch.Tensor, rows_per_rank: int, total_rows: int, world: int, cap: int, send: torch.Tensor,
               slot: torch.Tensor, counts: torch.Tensor, overflow: torch.Tensor):
    """Owner bucketing of a batch's ids for a row-sharded table (ncf_bucket_ids): fills ``send`` (world*cap,) int64 with
    local row ids (unused slots 0), ``slot`` (B,) int64 with each pair's row in the exchanged buffer (-1 = dropped),
    ``counts`` (world,) int32; sets the sticky out-of-range flag / ``overflow`` (int32 (1,)) on the device.  No host sync."""
    lib = load_library()
    _dev(idx, "idx")
    idx = _idx(idx)
    B = idx.numel()
    if send.dtype != torch.int64 or send.numel() < world * cap or slot.dtype != torch.int64 or slot.numel() < B \
            or counts.dtype != torch.int32 or counts.numel() < world or overflow.dtype != torch.int32:
        raise ValueError("bucket_ids: send / slot must be int64 of world*cap / B elements, counts / overflow int32")
    _check(lib.ncf_bucket_ids(_ptr(idx), B, int(rows_per_rank), int(total_rows), int(world), int(cap), _ptr(send), _ptr(slot),
                              _ptr(counts), _ptr(_oob_flag(idx.device)), _ptr(overflow), _stream(idx)))
    return send, slot, counts


def bucket_dedup_table_slots(B: int) -> int:
    return int(load_library().ncf_bucket_dedup_table_slots(int(B)))


def bucket_ids_dedup(idx: torch.Tensor, rows_per_rank: int, total_rows: int, world: int, cap: int, send: torch.Tensor,
                     slot: torch.Tensor, counts: torch.Tensor, overflow: torch.Tensor, hkeys: torch.Tensor, hvals: torch.Tensor):
    """ncf_bucket_ids_dedup: owner bucketing with every DISTINCT id listed once.  ``send`` (world*(cap+1),) int64 = buckets of
    [count, ids...]; ``slot`` (B,) int64 = each pair's row in the exchanged (world*cap)-row buffer (-1 = dropped); ``counts`` (world,)
    int32 = distinct ids per owner (may exceed cap); ``hkeys`` / ``hvals``: int64 scratch of bucket_dedup_table_slots(B) slots.
    Sticky flags on the device, no host sync."""
    lib = load_library()
    _dev(idx, "idx")
    idx = _idx(idx)
    B = idx.numel()
    H = min(hkeys.numel(), hvals.numel())
    if (send.dtype != torch.int64 or send.numel() < world * (cap + 1) or slot.dtype != torch.int64 or slot.numel() < B
            or counts.dtype != torch.int32 or counts.numel() < world or overflow.dtype != torch.int32
            or hkeys.dtype != torch.int64 or hvals.dtype != torch.int64):
        raise ValueError("bucket_ids_dedup: send / slot / hkeys / hvals must be int64 (world*(cap+1) / B / table slots), counts / overflow int32")
    Hp = 1 << (H.bit_length() - 1)        # the largest power of two the scratch holds
    _check(lib.ncf_bucket_ids_dedup(_ptr(idx), B, int(rows_per_rank), int(total_rows), int(world), int(cap), _ptr(hkeys), _ptr(hvals), Hp,
                                    _ptr(send), _ptr(slot), _ptr(counts), _ptr(_oob_flag(idx.device)), _ptr(overflow), _stream(idx)))
    return send, slot, counts


def gather_buckets(table: torch.Tensor, recv: torch.Tensor, world: int, cap: int, out: torch.Tensor) -> torch.Tensor:
    """ncf_gather_buckets: out[r * cap + k] = table[recv[r][1 + k]] for k < recv[r][0] (buckets of [count, ids...]); padding untouched."""
    lib = load_library()
    _dev(table, "table")
    rows, E, ld = _rows2d(table, "table")
    if recv.dtype != torch.int64 or recv.numel() < world * (cap + 1) or out.dtype != table.dtype or out.shape[0] < world * cap or out.shape[1] != E:
        raise ValueError("gather_buckets: recv must be int64 (world*(cap+1),) and out (world*cap, E) of the table's dtype")
    _check(lib.ncf_gather_buckets(_dt(table), _ptr(table), rows, ld, _ptr(recv), int(world), int(cap), E, _ptr(out), out.stride(0),
                                  _ptr(_oob_flag(table.device)), _stream(table)))
    return out


# ------------------------------------------------------------------ K2 generic
def _dims_array(dims: Sequence[int]):
    return (ctypes.c_int * len(dims))(*[int(d) for d in dims])


def _ptr_array(ts: Sequence[Optional[torch.Tensor]]):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def mlp_forward(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act chain: Linear, (ReLU, Linear)* — no activation after the last layer.  Any dims, fp32."""
    lib = load_library()
    _dev(x, "x")
    if x.dtype != torch.float32:
        raise TypeError(f"mlp_forward computes in fp32; got activations of dtype {x.dtype}")
    B, K0, ldx = _rows2d(x, "x")
    dims = [K0] + [int(w.shape[0]) for w in weights]
    for i, w in enumerate(weights):
        _dev(w, "weight")
        if w.dtype != torch.float32 or not w.is_contiguous() or w.shape[1] != dims[i]:
            raise ValueError(f"weight {i} must be contiguous fp32 [{dims[i + 1]}, {dims[i]}]")
    biases = [None if b is None else b.contiguous() for b in biases]
    n = len(weights)
    d = _dims_array(dims)
    ws_bytes = lib.ncf_mlp_workspace_bytes(NCF_F32, B, n, d)
    ws = _workspace(ws_bytes, x.device)
    if out is None:
        out = torch.empty((B, dims[-1]), dtype=torch.float32, device=x.device)
    _, _, ldo = _rows2d(out, "out")
    _check(lib.ncf_mlp_forward(NCF_F32, _ptr(x), B, ldx, n, d, _ptr_array(weights), _ptr_array(biases), _ptr(ws), ws_bytes,
                               _ptr(out), ldo, _stream(x)))
    return out


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
    return mlp_forward(x, [weight], [bias], out=out)


# ------------------------------------------------------------------ K1+K2 fused
class PackedMLP:
    """Weights of an MLP ending in a 1-wide layer, pre-packed for ncf_score_fused (built once per model)."""

    def __init__(self, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], dtype=torch.float32):
        """``dtype`` selects the kernel family: float32 (exact fp32 MFMA chain) or bfloat16 (weights rounded to bf16
        at pack time, bf16 tables, fp32 accumulate).  Sources are always fp32 [out][in] tensors."""
        lib = load_library()
        self.dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
        self.n_layers = len(weights)
        self.device = weights[0].device
        self.dtype = dtype
        self.dt = NCF_F32 if dtype == torch.float32 else NCF_BF16
        d = _dims_array(self.dims)
        nbytes = lib.ncf_mlp_packed_bytes(self.dt, self.n_layers, d)
        if nbytes == 0:
            raise NativeError(NCF_EUNSUPPORTED, "MLP shape cannot be packed for the fused kernel")
        ws = [w.detach().to(torch.float32).contiguous() for w in weights]
        bs = [None if b is None else b.detach().to(torch.float32).contiguous() for b in biases]
        for w in ws:
            _dev(w, "weight")
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        _check(lib.ncf_mlp_pack(self.dt, self.n_layers, d, _ptr_array(ws), _ptr_array(bs), _ptr(self.blob), nbytes,
                                _stream(ws[0])))

    def supports(self, EA: int, EB: int) -> bool:
        return bool(load_library().ncf_score_fused_supported(self.dt, EA, EB, self.n_layers, _dims_array(self.dims)))


def fused_supported(EA: int, EB: int, dims: Sequence[int], dtype=torch.float32) -> bool:
    dt = NCF_F32 if dtype == torch.float32 else NCF_BF16
    return bool(load_library().ncf_score_fused_supported(dt, EA, EB, len(dims) - 1, _dims_array(dims)))


def score_fused(tabA: torch.Tensor, idxA, tabB: Optional[torch.Tensor], idxB, packed: PackedMLP,
                out: Optional[torch.Tensor] = None, B: Optional[int] = None) -> torch.Tensor:
    lib = load_library()
    _dev(tabA, "tabA")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    rowsB = EB = ldB = 0
    if tabB is not None:
        _dev(tabB, "tabB")
        rowsB, EB, ldB = _rows2d(tabB, "tabB")
    idxA, idxB = _idx(idxA), _idx(idxB)
    if B is None:
        B = idxA.numel() if idxA is not None else (idxB.numel() if idxB is not None else rowsA)
    if out is None:
        out = torch.empty((B, 1), dtype=torch.float32, device=tabA.device)
    if tabA.dtype != packed.dtype:
        raise TypeError(f"tables are {tabA.dtype} but the MLP was packed for {packed.dtype}")
    _check(lib.ncf_score_fused(_dt(tabA), _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(idxA), _ptr(idxB), B, EA, EB,
                               packed.n_layers, _dims_array(packed.dims), _ptr(packed.blob), _ptr(out),
                               _ptr(_oob_flag(tabA.device)), _stream(tabA)))
    return out


def partial_supported(EA: int, EB: int, packed: PackedMLP) -> bool:
    """ncf_score_fused_partial has a kernel for tables of EA / EB columns scored by ``packed`` (fp32 only)."""
    return packed.dt == NCF_F32 and bool(load_library().ncf_score_fused_partial_supported(
        NCF_F32, int(EA), int(EB), packed.n_layers, _dims_array(packed.dims)))


def partial_in_lds(EA: int, EB: int, packed: PackedMLP) -> bool:
    """The partial kernel of this shape reads layer 1's weights from LDS (else it streams them, or there is none)."""
    return packed.dt == NCF_F32 and bool(load_library().ncf_score_fused_partial_in_lds(
        NCF_F32, int(EA), int(EB), packed.n_layers, _dims_array(packed.dims)))


def layer1_partial(tabA: torch.Tensor, packed: PackedMLP, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P (rowsA + 1, N1) fp32: layer 1's accumulators after table A's k-groups, for every row of ``tabA`` and (last row) for an
    out-of-range id — what score_fused_partial starts from.  Depends on tabA and the packed W1 / b1 only: build once per weight
    version.  Current stream, no sync."""
    lib = load_library()
    _dev(tabA, "tabA")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    EB, N1 = packed.dims[0] - EA, packed.dims[1]
    if out is None:
        out = torch.empty((rowsA + 1, N1), dtype=torch.float32, device=tabA.device)
    if out.shape[0] < rowsA + 1 or out.shape[1] < N1:
        raise ValueError(f"layer1_partial: out must hold ({rowsA + 1}, {N1}) floats")
    _, _, ldP = _rows2d(out, "out")
    _check(lib.ncf_layer1_partial(_dt(tabA), _ptr(tabA), rowsA, ldA, EA, EB, packed.n_layers, _dims_array(packed.dims),
                                  _ptr(packed.blob), _ptr(out), ldP, _stream(tabA)))
    return out


def score_fused_partial(P: torch.Tensor, tabA: torch.Tensor, idxA, tabB: torch.Tensor, idxB, packed: PackedMLP,
                        out: Optional[torch.Tensor] = None, B: Optional[int] = None) -> torch.Tensor:
    """Bit for bit score_fused(tabA, idxA, tabB, idxB, packed), with layer 1 started from P = layer1_partial(tabA, packed)."""
    lib = load_library()
    _dev(tabA, "tabA"), _dev(tabB, "tabB"), _dev(P, "P")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    rowsB, EB, ldB = _rows2d(tabB, "tabB")
    _, _, ldP = _rows2d(P, "P")
    if P.dtype != torch.float32 or P.shape[0] != rowsA + 1 or P.shape[1] != packed.dims[1]:
        raise ValueError(f"P must be fp32 ({rowsA + 1}, {packed.dims[1]}), built by layer1_partial from this tabA")
    idxA, idxB = _idx(idxA), _idx(idxB)
    if B is None:
        B = idxA.numel() if idxA is not None else (idxB.numel() if idxB is not None else rowsA)
    if out is None:
        out = torch.empty((B, 1), dtype=torch.float32, device=tabA.device)
    if tabA.dtype != packed.dtype:
        raise TypeError(f"tables are {tabA.dtype} but the MLP was packed for {packed.dtype}")
    _check(lib.ncf_score_fused_partial(_dt(tabA), _ptr(P), ldP, _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(idxA),
                                       _ptr(idxB), B, EA, EB, packed.n_layers, _dims_array(packed.dims), _ptr(packed.blob),
                                       _ptr(out), _ptr(_oob_flag(tabA.device)), _stream(tabA)))
    return out


# ------------------------------------------------------------------ K4 / K5
def spmm_csr(segptr: torch.Tensor, row_of: Optional[torch.Tensor], col: torch.Tensor, coef: Optional[torch.Tensor],
             z: torch.Tensor, N: int, y: Optional[torch.Tensor] = None, acc_sum: Optional[torch.Tensor] = None,
             partial: Optional[torch.Tensor] = None, fixup: bool = True, dropout: Optional[tuple] = None) -> torch.Tensor:
    """``dropout`` = (p, seed, edge_id or None): per-(edge, feature) message dropout regenerated in the kernel (training)."""
    lib = load_library()
    _dev(z, "z")
    Nz, D, ldz = _rows2d(z, "z")
    n_seg = segptr.numel() - 1
    if segptr.dtype != torch.int64 or col.dtype != torch.int32:
        raise TypeError("segptr must be int64 and col int32")
    if row_of is not None and row_of.dtype != torch.int32:
        raise TypeError("row_of must be int32")
    if y is None:
        y = torch.empty((N, D), dtype=torch.float32, device=z.device)
    if row_of is not None and partial is None:
        partial = torch.empty((n_seg, D), dtype=torch.float32, device=z.device)
    args = (NCF_F32, _ptr(segptr), _ptr(row_of), n_seg, _ptr(col), _ptr(coef), _ptr(z), Nz, ldz, D, _ptr(y), y.stride(0), _ptr(acc_sum),
            0 if acc_sum is None else acc_sum.stride(0), _ptr(partial), 1 if fixup else 0)
    if dropout is not None and dropout[0] > 0:
        p, seed, eid = dropout
        if eid is not None and (eid.dtype != torch.int32 or eid.numel() != col.numel()):
            raise TypeError("edge ids must be int32, one per CSR entry")
        _check(lib.ncf_spmm_csr_dropout(*args, _ptr(eid), int(seed) & 0xFFFFFFFF, float(p), _stream(z)))
    else:
        _check(lib.ncf_spmm_csr(*args, _stream(z)))
    return y


class SegmentedCSR:
    """A CSR-by-destination matrix prepared for ncf_spmm_csr: rows longer than ``seg_len`` edges are split into
    segments (load balance), and rows with more than one segment are finished by re-applying the SAME kernel to the
    partial sums with ``fan``-wide segments, level after level, until one segment per row is left — an ordered
    log-depth tree (a hub item with 4 M in-edges: 8 k partials -> 125 -> 2 -> 1) instead of one lane group walking
    8 k partials serially.  Deterministic: every level adds in index order."""

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, coef: Optional[torch.Tensor], seg_len: int = 512, fan: int = 64):
        self.n_rows = rowptr.numel() - 1
        self.col, self.coef = col, coef
        counts = rowptr[1:] - rowptr[:-1]
        self._build_tree(rowptr, counts, seg_len, fan)

    @staticmethod
    def _split(rowptr, row_ids, counts, seg_len):
        """Segments of at most seg_len edges per row.  Returns (segptr, row_of or None, nseg per row)."""
        dev = rowptr.device
        nseg = torch.clamp((counts + seg_len - 1) // seg_len, min=1)
        n = counts.numel()
        if n == 0 or int(nseg.max()) == 1:
            return rowptr, None, nseg
        local_row = torch.repeat_interleave(torch.arange(n, device=dev), nseg)
        first = torch.cumsum(nseg, 0) - nseg
        local = torch.arange(local_row.numel(), device=dev) - first[local_row]
        segptr = torch.empty(local_row.numel() + 1, dtype=torch.int64, device=dev)
        segptr[:-1] = rowptr[local_row] + local * seg_len
        segptr[-1] = rowptr[-1]
        return segptr, row_ids[local_row].to(torch.int32).contiguous(), nseg

    def _build_tree(self, rowptr, counts, seg_len, fan):
        dev = rowptr.device
        self.levels = []
        row_ids = torch.arange(self.n_rows, device=dev)
        segptr, row_of, nseg = self._split(rowptr, row_ids, counts, seg_len)
        self.levels.append((segptr, row_of, None))
        while row_of is not None:
            # segments of this level that belong to multi-segment rows are the next level's "edges"
            local_row = torch.repeat_interleave(torch.arange(nseg.numel(), device=dev), nseg)
            multi_seg = (nseg > 1)[local_row]
            edge_ids = torch.nonzero(multi_seg).flatten()                 # ids into this level's partial buffer
            keep_rows = nseg > 1
            row_ids = row_ids[keep_rows]
            counts = nseg[keep_rows]
            rp = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
            rp[1:] = torch.cumsum(counts, 0)
            segptr, row_of, nseg = self._split(rp, row_ids, counts, fan)
            if row_of is None:  # every remaining row fits one segment: the kernel still needs the row map
                row_of_last = row_ids.to(torch.int32).contiguous()
                self.levels.append((segptr, row_of_last, edge_ids.to(torch.int32).contiguous()))
                break
            self.levels.append((segptr, row_of, edge_ids.to(torch.int32).contiguous()))
        self._partials = {}

    def spmm(self, z: torch.Tensor, y: Optional[torch.Tensor] = None, acc_sum: Optional[torch.Tensor] = None,
             coef: Optional[torch.Tensor] = None, dropout: Optional[tuple] = None) -> torch.Tensor:
        """``coef`` overrides the per-edge coefficients for this call (LightGAT recomputes them every layer; a training step
        masks target edges).  ``dropout`` = (p, seed, edge_id or None): message dropout at the edge level (see spmm_csr)."""
        D = z.shape[1]
        coef = self.coef if coef is None else coef
        segptr, row_of, _ = self.levels[0]
        if y is None:
            y = torch.empty((self.n_rows, D), dtype=torch.float32, device=z.device)
        if len(self.levels) == 1:
            return spmm_csr(segptr, row_of, self.col, coef, z, self.n_rows, y=y, acc_sum=acc_sum, dropout=dropout)
        bufs = self._partials.get(D)
        if bufs is None:
            bufs = [torch.empty((lv[0].numel() - 1, D), dtype=torch.float32, device=z.device) for lv in self.levels[:-1]]
            self._partials[D] = bufs
        spmm_csr(segptr, row_of, self.col, coef, z, self.n_rows, y=y, acc_sum=acc_sum, partial=bufs[0], fixup=False, dropout=dropout)
        for li in range(1, len(self.levels)):
            segptr, row_of, edge_ids = self.levels[li]
            last = li == len(self.levels) - 1
            spmm_csr(segptr, row_of, edge_ids, None, bufs[li - 1], self.n_rows, y=y, acc_sum=acc_sum,
                     partial=None if last else bufs[li], fixup=False)
        return y


def degree_accumulate(dst: torch.Tensor, N: int, deg: torch.Tensor):
    lib = load_library()
    _dev(dst, "dst")
    _check(lib.ncf_degree_accumulate(_ptr(dst), dst.numel(), N, _ptr(deg), _ptr(_oob_flag(dst.device)), _stream(dst)))
    return deg


def edge_coef(src: torch.Tensor, dst: torch.Tensor, attr: Optional[torch.Tensor], deg: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    _dev(src, "src")
    coef = torch.empty(src.numel(), dtype=torch.float32, device=src.device)
    _check(lib.ncf_edge_coef(_ptr(src), _ptr(dst), _ptr(attr), _ptr(deg), src.numel(), deg.numel(), _ptr(coef), _stream(src)))
    return coef


def edge_keep(segptr: torch.Tensor, row_of: Optional[torch.Tensor], N: int, col: torch.Tensor, attr: Optional[torch.Tensor],
              pair_key: Optional[torch.Tensor] = None, targets_sorted: Optional[torch.Tensor] = None, slot: Optional[torch.Tensor] = None,
              p: float = 0.0, seed: int = 0, node_keep: Optional[torch.Tensor] = None):
    """The edges one training step keeps (ncf_edge_keep, "THE KEEP RULE" of include/ncf_abi.h) over the level-0 segments of a CSR by
    destination: returns (w (E,) float32 = the entry's weight where kept, 0 where removed; deg (N,) int32 = kept entries per row).
    ``targets_sorted``: ascending user * N + item keys of the batch (None / empty: no target masking); ``slot`` / ``p`` / ``seed``:
    message dropout; ``node_keep``: (N,) uint8 mask of node dropout (None: every node kept)."""
    lib = load_library()
    _dev(col, "col")
    E = col.numel()
    if segptr.dtype != torch.int64 or col.dtype != torch.int32 or not segptr.is_contiguous() or not col.is_contiguous():
        raise TypeError("segptr must be contiguous int64 and col contiguous int32")
    if row_of is not None and row_of.dtype != torch.int32:
        raise TypeError("row_of must be int32")
    n_seg = segptr.numel() - 1
    if row_of is not None and row_of.numel() != n_seg:
        raise ValueError("row_of must hold one row per segment")
    if row_of is None and n_seg != N:
        raise ValueError("without row_of the segments are the N rows")
    n_targets = 0 if targets_sorted is None else targets_sorted.numel()
    for t, dt, what in ((attr, torch.float32, "attr"), (slot, torch.int32, "slot"), (pair_key, torch.int64, "pair_key")):
        if t is not None and (t.dtype != dt or t.numel() != E or not t.is_contiguous()):
            raise TypeError(f"{what} must be contiguous {dt}, one element per CSR entry")
    if n_targets and (targets_sorted.dtype != torch.int64 or not targets_sorted.is_contiguous()):
        raise TypeError("targets_sorted must be contiguous int64")
    if node_keep is not None and (node_keep.dtype != torch.uint8 or node_keep.numel() != N or not node_keep.is_contiguous()):
        raise TypeError("node_keep must be contiguous uint8, one byte per node")
    w = torch.empty(E, dtype=torch.float32, device=col.device)
    deg = torch.empty(N, dtype=torch.int32, device=col.device)
    if E == 0:                                # an edgeless graph: nothing to keep, and empty tensors carry null pointers
        return w, deg.zero_()
    _check(lib.ncf_edge_keep(_ptr(segptr), _ptr(row_of), n_seg, N, _ptr(col), _ptr(attr), _ptr(pair_key),
                             _ptr(targets_sorted) if n_targets else None, n_targets, _ptr(slot), float(p), int(seed) & 0xFFFFFFFF,
                             _ptr(node_keep), _ptr(w), _ptr(deg), _stream(col)))
    return w, deg


def scale_rows(x: torch.Tensor, divisor: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load_library()
    _dev(x, "x")
    N, D, ld = _rows2d(x, "x")
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=x.device)
    _check(lib.ncf_scale_rows(_ptr(x), ld, N, D, float(divisor), _ptr(out), out.stride(0), _stream(x)))
    return out


# ------------------------------------------------------------------ K3
def _attn_operands(mode, pc, pr, w1, csr=None, feat=None, checked=True):
    """The operands the attention entry points share: ((mode, pc, ldpc, pr, ldpr, A, w1) as the ABI takes them — b1 follows where an
    entry has one —, the pointers of the CSR triple, (feat, ldf, Fdim), (B, I, A, Fdim)).  ``checked``: the operands must agree and
    the CSR be (int64, int32, fp32); attn_backward takes what its forward checked."""
    _dev(pc, "pc")
    B, A, ldpc = _rows2d(pc, "pc")
    I, A2, ldpr = _rows2d(pr, "pr")
    I2, Fdim, ldf = (I, 0, 0) if feat is None else _rows2d(feat, "feat")
    if checked:
        if A != A2 or I != I2:
            raise ValueError("attention operand shapes disagree")
        if csr is not None and (csr[0].dtype != torch.int64 or csr[1].dtype != torch.int32 or csr[2].dtype != torch.float32):
            raise TypeError("CSR must be (int64 rowptr, int32 col, fp32 val)")
    return ((mode, _ptr(pc), ldpc, _ptr(pr), ldpr, A, _ptr(w1)), () if csr is None else (_ptr(csr[0]), _ptr(csr[1]), _ptr(csr[2])),
            (_ptr(feat), ldf, Fdim), (B, I, A, Fdim))


def attn_forward(mode: int, pc: torch.Tensor, pr: torch.Tensor, w1: Optional[torch.Tensor], b1: float,
                 rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, feat: torch.Tensor,
                 out_bias: Optional[torch.Tensor] = None, dropout: Optional[tuple] = None, msg_dropout: Optional[tuple] = None):
    """Returns (out_feat (B, Fdim), weights (nnz,)).  ``dropout`` = (p, seed): AttentionNet's hidden dropout (training);
    ``msg_dropout`` = (p, seed): the message dropout over the (pair, rated entry) logits (ncf_attn_forward_train; ``b1`` then takes
    part in the reference's ``== 0`` test).  None or p == 0 for it: exactly the calls made without the argument."""
    lib = load_library()
    head, csr, ft, (B, I, _, Fdim) = _attn_operands(mode, pc, pr, w1, (rowptr, col, val), feat)
    out = torch.empty((B, Fdim), dtype=torch.float32, device=pc.device)
    wts = torch.empty(max(col.numel(), 1), dtype=torch.float32, device=pc.device)
    if msg_dropout is not None and msg_dropout[0] > 0:
        p, seed = dropout if dropout is not None else (0.0, 0)
        fn, draws = lib.ncf_attn_forward_train, (int(seed) & 0xFFFFFFFF, float(p), int(msg_dropout[1]) & 0xFFFFFFFF, float(msg_dropout[0]))
    elif dropout is not None and dropout[0] > 0:
        fn, draws = lib.ncf_attn_forward_dropout, (int(dropout[1]) & 0xFFFFFFFF, float(dropout[0]))
    else:
        fn, draws = lib.ncf_attn_forward, ()
    _check(fn(*head, float(b1), *csr, B, I, *ft, _ptr(out_bias), _ptr(out), out.stride(0), _ptr(wts), *draws, _stream(pc)))
    return out, wts[:col.numel()]


def attn_backward(mode: int, pc, pr, w1, rowptr, col, val, feat, wts, dout, dropout: Optional[tuple] = None,
                  msg_dropout: Optional[tuple] = None):
    """Gradients of attn_forward: (d_pc (B, A), d_pr (I, A), d_w1 (A,) or None, d_feat (I, Fdim)); d b1 is exactly zero.
    ``msg_dropout`` = the forward's (p, seed): only p is used (ncf_attn_backward_train needs no mask)."""
    lib = load_library()
    head, csr, ft, (B, I, A, Fdim) = _attn_operands(mode, pc, pr, w1, (rowptr, col, val), feat, checked=False)
    dout = dout.contiguous()
    d_pc = torch.empty((B, A), dtype=torch.float32, device=pc.device)
    d_pr = torch.zeros((I, A), dtype=torch.float32, device=pc.device)
    d_feat = torch.zeros((I, Fdim), dtype=torch.float32, device=pc.device)
    mlp = mode in (ATT_MLP, ATT_MLP_SCALED)
    part = torch.empty((B, A), dtype=torch.float32, device=pc.device) if mlp else None
    scratch = torch.empty(max(col.numel(), 1), dtype=torch.float32, device=pc.device)
    p, seed = (dropout if dropout is not None else (0.0, 0))
    if msg_dropout is not None and msg_dropout[0] > 0:
        fn, draws = lib.ncf_attn_backward_train, (float(msg_dropout[0]),)
    else:
        fn, draws = lib.ncf_attn_backward, ()
    _check(fn(*head, *csr, B, I, *ft, _ptr(wts), _ptr(dout), dout.stride(0), _ptr(d_pc), A, _ptr(d_pr), A, _ptr(part), _ptr(d_feat), Fdim,
              _ptr(scratch), int(seed) & 0xFFFFFFFF, float(p), *draws, _stream(pc)))
    return d_pc, d_pr, (colsum(part) if mlp and B > 0 else (torch.zeros(A, device=pc.device) if mlp else None)), d_feat


def attn_grouped_supported(mode: int, A: int, Fdim: int) -> bool:
    """Shapes the LDS-tiled grouped kernel takes (mirrors ncf_attn_forward_grouped's NCF_EUNSUPPORTED conditions)."""
    return mode in (ATT_MLP, ATT_COS, ATT_MLP_SCALED) and A % 4 == 0 and A <= 256 and Fdim <= 256


ATTN_GROUPED_FORMS = {0: "none", 1: "sc", 2: "lds"}    # ncf_attn_grouped_plan's *form


def attn_grouped_plan(mode: int, A: int, Fdim: int, ldfeat: Optional[int] = None, pairs_per_wg: int = 16, B: int = 1, n_rows: int = 1):
    """(form, kernel MODE, CPB or FO, NW or NPF, LDS bytes, grid_x) of the kernel ncf_attn_forward_grouped runs for the shape under
    the current attn_grouped_kernel option; form by name (ATTN_GROUPED_FORMS): "sc" = attn_grouped_sc_kernel<MODE, CPB, NW>, "lds" =
    attn_grouped_kernel<MODE, FO, NPF>.  Host only: no launch, no device.  Raises NativeError where the launch would refuse."""
    form, *rest = _query(load_library().ncf_attn_grouped_plan,
                         (int(mode), int(A), int(Fdim), int(Fdim if ldfeat is None else ldfeat), int(pairs_per_wg), int(B), int(n_rows)),
                         (_c_int, _c_int, _c_int, _c_int, _c_i64, _c_i64))
    return (ATTN_GROUPED_FORMS[form], *rest)


def attn_backward_supported(mode: int, A: int, Fdim: int) -> bool:
    """Shapes the training pair ``ncf_attn_forward`` + ``ncf_attn_backward`` takes: mirrors ncf_attn_backward's own
    NCF_EUNSUPPORTED conditions (csrc/attn.hip: MLP / cosine only; A and Fdim multiples of 4 and <= 256 — the leading
    dimensions are those of contiguous (.., A) / (.., Fdim) tensors, so they are multiples of 4 when A and Fdim are).  The
    plain forward accepts any Fdim through its generic path, so a gate on the forward's conditions would let
    ``loss.backward()`` raise for e.g. user_emb = 50."""
    return mode in (ATT_MLP, ATT_COS, ATT_MLP_SCALED) and A % 4 == 0 and Fdim % 4 == 0 and 0 < A <= 256 and 0 < Fdim <= 256


def default_pairs_per_wg(B: int) -> int:
    """Pairs of one rated set per workgroup of the grouped attention kernel (4 per wave).  32 (512 threads) stages a tile
    for twice as many pairs as 16 (256 threads): half the gathered bytes per pair, and the tile DMAs hold a wave for about a
    third of a tile's time.  Measured (tools/ab_attn_grouped.py, scalar-operand form, 8 / 16 / 32): config 3 (4096 pairs, 64
    users) 59.2 / 37.9 / 34.4 us; 16 384 pairs 137.8 / 94.4 / 97.1; one user x 65 536 candidates 450.6 / 261.8 / 240.9."""
    return 32 if B >= 2048 else (16 if B >= 512 else 8)


def group_pairs(pair_row: torch.Tensor, n_rows: int, pairs_per_wg: int):
    """Pairs listed row by row for ncf_attn_forward_grouped: (grp_ptr (R+1), pair_ids (B), wg_ptr (R+1)), all int64 on
    pair_row's device — a counting sort on the stream (ncf_group_pairs), no host synchronisation; an out-of-range row
    raises at the next check_oob()."""
    lib = load_library()
    _dev(pair_row, "pair_row")
    if pair_row.dtype != torch.int64 or pair_row.dim() != 1 or not pair_row.is_contiguous():
        raise ValueError("pair_row must be contiguous 1-D int64")
    B, R, dev = pair_row.numel(), int(n_rows), pair_row.device
    grp_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
    wg_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
    pair_ids = torch.empty(max(B, 1), dtype=torch.int64, device=dev)
    # workgroup -> CSR row (the grid bound of the grouped kernels: every non-empty row adds at most one partly filled workgroup)
    wg_row = torch.empty((B + int(pairs_per_wg) - 1) // int(pairs_per_wg) + min(R, B) + 1, dtype=torch.int32, device=dev)
    nbytes = lib.ncf_group_pairs_workspace_bytes(R)
    ws = _workspace(nbytes, dev)
    _check(lib.ncf_group_pairs_rows(_ptr(pair_row), B, R, int(pairs_per_wg), _ptr(grp_ptr), _ptr(pair_ids), _ptr(wg_ptr), _ptr(wg_row),
                                    _ptr(ws), nbytes, _ptr(_oob_flag(dev)), _stream(pair_row)))
    return Grouping(grp_ptr, pair_ids[:B], wg_ptr, wg_row)


class Grouping(tuple):
    """(grp_ptr, pair_ids, wg_ptr) of ncf_group_pairs — unpacks as that triple — plus ``wg_row`` (workgroup -> CSR row)."""

    def __new__(cls, grp_ptr, pair_ids, wg_ptr, wg_row=None):
        self = super().__new__(cls, (grp_ptr, pair_ids, wg_ptr))
        self.wg_row = wg_row
        return self


DENSE_CSR_MAX_ENTRIES = 1 << 26     # col / val are sized for the worst case B * I: beyond 64 M entries the host-sized path is used


def dense_to_csr(user_matrix: torch.Tensor, share_rows: bool = True):
    """(rowptr (B+1) int64, col int32, val fp32, pair_row (B) int64) of a dense (B, I) user_matrix, entirely on the stream
    (ncf_dense_csr_rows + cumsum + ncf_dense_csr_fill; no host read).  The CSR has B rows; with ``share_rows`` a row that equals an
    earlier one is empty and pair_row points at the earlier one.  col / val are sized B * I (only rowptr[B] entries are written)."""
    lib = load_library()
    _dev(user_matrix, "user_matrix")
    if user_matrix.dtype != torch.float32:
        raise TypeError("dense_to_csr takes an fp32 matrix")
    B, I, ld = _rows2d(user_matrix, "user_matrix")
    dev = user_matrix.device
    pair_row = torch.empty(B, dtype=torch.int64, device=dev)
    col = torch.empty(max(B * I, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(B * I, 1), dtype=torch.float32, device=dev)
    if B == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev), col, val, pair_row
    rowptr = torch.empty(B + 1, dtype=torch.int64, device=dev)     # [0, counts...] from the kernels; the cumulative sum runs in place
    nbytes = lib.ncf_dense_csr_workspace_bytes(B)
    ws = _workspace(nbytes, dev)
    _check(lib.ncf_dense_csr_rows(_ptr(user_matrix), ld, B, I, 1 if share_rows else 0, _ptr(pair_row), _ptr(rowptr), _ptr(ws), nbytes, _stream(user_matrix)))
    torch.cumsum(rowptr, 0, out=rowptr)
    _check(lib.ncf_dense_csr_fill(_ptr(user_matrix), ld, B, I, _ptr(rowptr), _ptr(pair_row), _ptr(col), _ptr(val), _stream(user_matrix)))
    return rowptr, col, val, pair_row


def _pair_rows_flag(device) -> torch.Tensor:
    """The sticky overflow flag of pair_rows calls that run inside a training step (nobody reads a per-call flag there)."""
    return _flag("pair_rows", device)


def check_pair_rows(device):
    """Synchronising check of the sticky flag a pair_rows call sets when a pair's entries did not fit its capacity."""
    _check_flag("pair_rows", device)


def pair_rows(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, pair_row: torch.Tensor, capacity: int, mask=None,
              atol: float = 1e-5, rtol: float = 1e-5, flag: Optional[torch.Tensor] = None):
    """(out_rowptr (B+1) int64, out_col int32, out_val fp32, flag int32[1]): the per-pair CSR of a shared-row CSR (pair b uses row
    ``pair_row[b]``), entirely on the stream (ncf_pair_rows_count + cumsum + ncf_pair_rows_fill; no host read).  out_col / out_val
    hold ``capacity`` entries, of which out_rowptr[B] are written; an entry past capacity is dropped, out_rowptr is cut off at
    capacity (the CSR stays consistent with its buffers) and ``flag`` is set (int32[1]: a fresh zero unless the caller passes one to accumulate in, e.g. ``_pair_rows_flag``; it is never cleared here).  ``mask`` = (cand_emb (B, E), rated_emb (I, E)): AttentionNCF's
    train-only target mask — out_col = -1 where the pair's candidate row is torch.isclose (fp32, ``atol`` / ``rtol``) to the rated
    item's in every element.  A pair_row outside the CSR gives an empty row and sets the sticky out-of-range flag (check_oob)."""
    lib = load_library()
    _dev(rowptr, "rowptr")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float32:
        raise TypeError("pair_rows takes an int64 rowptr, int32 columns and fp32 values")
    if not (rowptr.is_contiguous() and col.is_contiguous() and val.is_contiguous()) or rowptr.numel() < 1:
        raise ValueError("pair_rows takes a contiguous CSR")
    pair_row = _idx(pair_row)
    R, B, capacity = rowptr.numel() - 1, pair_row.numel(), int(capacity)
    if capacity < 0:
        raise ValueError("capacity must be >= 0")
    dev = rowptr.device
    out_rowptr = torch.zeros(1, dtype=torch.int64, device=dev) if B == 0 else torch.empty(B + 1, dtype=torch.int64, device=dev)
    out_col = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
    out_val = torch.empty(max(capacity, 1), dtype=torch.float32, device=dev)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    elif flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != dev:
        raise ValueError("flag must be one int32 on the CSR's device")
    cand = rated = None
    I = E = ldc = ldr = 0
    if mask is not None:
        cand, rated = mask
        _dev(cand, "cand_emb"), _dev(rated, "rated_emb")
        if cand.dtype != torch.float32 or rated.dtype != torch.float32:
            raise TypeError("pair_rows compares fp32 embeddings")
        Bc, E, ldc = _rows2d(cand, "cand_emb")
        I, Er, ldr = _rows2d(rated, "rated_emb")
        if Bc != B or Er != E:
            raise ValueError(f"mask shapes {tuple(cand.shape)} / {tuple(rated.shape)} do not fit {B} pairs")
    if B == 0:
        return out_rowptr, out_col, out_val, flag
    st = _stream(rowptr)
    _check(lib.ncf_pair_rows_count(_ptr(rowptr), R, _ptr(pair_row), B, _ptr(out_rowptr), _ptr(_oob_flag(dev)), st))
    torch.cumsum(out_rowptr, 0, out=out_rowptr)
    _check(lib.ncf_pair_rows_fill(_ptr(rowptr), _ptr(col), _ptr(val), R, _ptr(pair_row), B, _ptr(out_rowptr), _ptr(out_col), _ptr(out_val),
                                  capacity, _ptr(cand), ldc, _ptr(rated), ldr, I, E, float(atol), float(rtol), _ptr(flag), st))
    # what did not fit was not written: the returned CSR ends at capacity (a truncated row, then empty ones), so that a kernel bounded
    # by rowptr never reads or writes past buffers sized like out_col, whatever the flag says when somebody looks
    torch.clamp(out_rowptr, max=capacity, out=out_rowptr)
    return out_rowptr, out_col, out_val, flag


def _events_us(fn, reps, settle):
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def probe_gather_ceilings(table: torch.Tensor, idx: torch.Tensor, copy_bytes: int, reps: int = 100):
    """What the chip delivers, now, for the two patterns the standalone gather is made of (ncf_probe_copy / ncf_probe_gather_read):
    a streaming copy of ``copy_bytes`` (read + write counted) and random whole-row reads of ``table`` rows named by ``idx`` (read
    bytes only) at 1 / 2 / 4 / 8 rows in flight per lane group and two grid sizes.  GB/s; the best of the sweep is the ceiling."""
    lib = load_library()
    _dev(table, "table")
    rows, E, ld = _rows2d(table, "table")
    rb = E * table.element_size()
    dev = table.device
    st = torch.cuda.current_stream(dev).cuda_stream
    src = torch.empty(copy_bytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    us = _events_us(lambda: _check(lib.ncf_probe_copy(_ptr(src), _ptr(dst), copy_bytes, st)), reps, 30)
    out = {"copy": {"bytes_read_plus_written": 2 * copy_bytes, "us": us, "GBps": 2 * copy_bytes / (us * 1e-6) / 1e9}, "random_row_read": {}}
    n = idx.numel()
    best = 0.0
    for blocks in (2048, 8192):
        sink = torch.empty(blocks * 256, dtype=torch.int32, device=dev)
        for u in (1, 2, 4, 8):
            us = _events_us(lambda: _check(lib.ncf_probe_gather_read(_ptr(table), rows, ld * table.element_size(), rb, _ptr(idx), n, u, blocks,
                                                                     _ptr(sink), st)), reps, 20)
            gbs = n * rb / (us * 1e-6) / 1e9
            out["random_row_read"][f"blocks{blocks}_inflight{u}"] = {"us": us, "GBps": gbs}
            best = max(best, gbs)
    out["random_row_read_best_GBps"] = best
    out["row_bytes"] = rb
    return out


def probe_mfma_bf16(device, seconds: float = 2.0, with_lds: bool = False, blocks: int = 256, iters: int = 20000):
    """The bf16 MFMA rate the chip sustains on random operands (ncf_probe_mfma_bf16): back-to-back launches for ``seconds`` (the
    clock needs about two seconds of load to settle), the LAST launches timed with HIP events.  Returns {"TFLOPs", "clock_GHz",
    "us_per_launch", ...}."""
    lib = load_library()
    g = torch.Generator(device=device).manual_seed(1234)
    rnd = (torch.randn(32768, device=device, generator=g) * 0.5).to(torch.bfloat16).contiguous()      # 64 KiB of finite bf16
    sink = torch.empty(blocks * 512, dtype=torch.float32, device=device)
    clk = torch.zeros(blocks * 8 * 2, dtype=torch.int64, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream

    def launch():
        _check(lib.ncf_probe_mfma_bf16(_ptr(rnd), int(iters), int(blocks), 1 if with_lds else 0, _ptr(sink), _ptr(clk), stream))

    flop = blocks * 8 * iters * 32 * 16384
    launch()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); launch(); e1.record()
    torch.cuda.synchronize(device)
    one = e0.elapsed_time(e1) * 1e-3
    n = max(4, int(seconds / max(one, 1e-6)))
    for _ in range(n - 4):
        launch()
    e0.record()
    for _ in range(4):
        launch()
    e1.record()
    torch.cuda.synchronize(device)
    us = e0.elapsed_time(e1) * 1e3 / 4
    c = clk.view(-1, 2).double().cpu()
    ghz = float((c[:, 0] / c[:, 1].clamp_min(1)).median()) * 0.1
    return {"TFLOPs": flop / (us * 1e-6) / 1e12, "clock_GHz": ghz, "us_per_launch": us, "launches": n, "blocks": blocks,
            "iters": iters, "with_lds_reads": bool(with_lds), "mfma": "v_mfma_f32_16x16x32_bf16, 2 waves per SIMD, register operands, random data",
            "cycles_per_mfma_per_simd": float(c[:, 0].median()) / (iters * 32 * 2)}      # two waves share a SIMD's matrix pipe


def attn_candidates_supported(K: int, N1: int, N2: int) -> bool:
    return bool(load_library().ncf_attn_candidates_supported(int(K), int(N1), int(N2)))


class PackedCandidateWeight:
    """ItemEmbeddings' (N1, K) weight in MFMA operand order for attn_candidates (ncf_attn_candidates_pack): built once per weight
    version (the model keeps it beside its other weight-derived caches)."""

    def __init__(self, Wi: torch.Tensor):
        lib = load_library()
        _dev(Wi, "Wi")
        if Wi.dtype != torch.float32:
            raise TypeError("attn_candidates computes in fp32")
        self.N1, self.K, ldw = _rows2d(Wi, "Wi")
        self.src = Wi
        # Both widths take the packed entry point at every batch size: measured (tools/ab_cand.py, us per call incl. the grouping;
        # LDS-staged -> packed): N1 = 64: 4096 rows 25.1 -> 20.5, 16 384 rows 96.7 -> 74.0; N1 = 128: 512 rows 29.3 -> 22.2 (K range
        # over workgroups), 4096 rows 41.3 -> 38.6, 16 384 rows 159.0 -> 141.5.  ``use_packed = False`` selects the LDS-staged kernel.
        self.use_packed = True
        self.data = torch.empty(lib.ncf_attn_candidates_pack_floats(self.K, self.N1), dtype=torch.float32, device=Wi.device)
        _check(lib.ncf_attn_candidates_pack(_ptr(Wi), ldw, self.K, self.N1, _ptr(self.data), _stream(Wi)))


def attn_candidates(x: torch.Tensor, Wi, bi: Optional[torch.Tensor], Wc: torch.Tensor, b0: Optional[torch.Tensor],
                    pair_row: Optional[torch.Tensor] = None, n_rows: int = 0, pairs_per_wg: int = 32):
    """ncf_attn_candidates: (emb (B, N1), pc (B, N2), grouping or None) — the candidates' ItemEmbeddings and their half of
    AttentionNet.0 in one launch; with ``pair_row`` (B,) int64 the same launch also lists the pairs by rated set (the ``Grouping``
    group_pairs() returns).  ``Wi``: the (N1, K) weight, or a PackedCandidateWeight of it (ncf_attn_candidates_packed: the faster
    form, bit-identical results).  Shapes: attn_candidates_supported(); the fused grouping needs B, n_rows <= 32768."""
    lib = load_library()
    _dev(x, "x")
    if isinstance(Wi, PackedCandidateWeight) and not Wi.use_packed:
        Wi = Wi.src
    packed = isinstance(Wi, PackedCandidateWeight)
    if x.dtype != torch.float32 or (not packed and Wi.dtype != torch.float32) or Wc.dtype != torch.float32:
        raise TypeError("attn_candidates computes in fp32")
    B, K, ldx = _rows2d(x, "x")
    if packed:
        N1, K2, ldw = Wi.N1, Wi.K, 0
    else:
        N1, K2, ldw = _rows2d(Wi, "Wi")
    N2 = int(Wc.shape[0])
    if K2 != K or Wc.shape[1] != N1 or not Wc.is_contiguous():
        raise ValueError("attn_candidates: Wi must be (N1, K) and Wc contiguous (N2, N1)")
    dev = x.device
    emb = torch.empty((B, N1), dtype=torch.float32, device=dev)
    pc = torch.empty((B, N2), dtype=torch.float32, device=dev)
    grp = None
    grp_ptr = pair_ids = wg_ptr = wg_row = ws = None
    nbytes = 0
    R = int(n_rows)
    if pair_row is not None:
        if pair_row.dtype != torch.int64 or pair_row.dim() != 1 or not pair_row.is_contiguous() or pair_row.numel() != B:
            raise ValueError("pair_row must be contiguous 1-D int64 with one entry per row of x")
        grp_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
        wg_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
        pair_ids = torch.empty(max(B, 1), dtype=torch.int64, device=dev)
        wg_row = torch.empty((B + int(pairs_per_wg) - 1) // int(pairs_per_wg) + min(R, B) + 1, dtype=torch.int32, device=dev)
        nbytes = lib.ncf_attn_candidates_workspace_bytes(R)
        grp = Grouping(grp_ptr, pair_ids[:B], wg_ptr, wg_row)
    if packed:
        nbytes = lib.ncf_attn_candidates_packed_workspace_bytes(B, N1, R if pair_row is not None else -1)
    if nbytes:                                # without a grouping the LDS-staged form has no scratch and takes a null pointer
        ws = _workspace(nbytes, dev)
    tail = (_ptr(bi), N1, _ptr(Wc), _ptr(b0), N2, _ptr(emb), emb.stride(0), _ptr(pc), pc.stride(0), _ptr(pair_row), R, int(pairs_per_wg),
            _ptr(grp_ptr), _ptr(pair_ids), _ptr(wg_ptr), _ptr(wg_row), _ptr(ws), nbytes,
            _ptr(_oob_flag(dev)) if pair_row is not None else None, _stream(x))
    if packed:
        _check(lib.ncf_attn_candidates_packed(_ptr(x), B, ldx, K, _ptr(Wi.data), *tail))
    else:
        _check(lib.ncf_attn_candidates(_ptr(x), B, ldx, K, _ptr(Wi), ldw, *tail))
    return emb, pc, grp


class AttnPartials:
    """The entry-split attention's un-merged softmax partials: (B, nsplit, Fdim + 4) floats in ``ws`` — what attn_tail() merges."""

    def __init__(self, ws, nsplit, Fdim, B):
        self.ws, self.nsplit, self.Fdim, self.B = ws, int(nsplit), int(Fdim), int(B)


def attn_tail_supported(EA: int, UE: int, N1: int, N2: int) -> bool:
    return bool(load_library().ncf_attn_tail_supported(int(EA), int(UE), int(N1), int(N2)))


class PackedTailWeight:
    """A hidden layer's (N, K) weight of the tail MLP in MFMA operand order (ncf_attn_tail_pack_weight), built once per weight version."""

    def __init__(self, W: torch.Tensor):
        lib = load_library()
        _dev(W, "W")
        if W.dtype != torch.float32 or W.dim() != 2 or not W.is_contiguous():
            raise TypeError("PackedTailWeight takes a contiguous fp32 (N, K) weight")
        self.shape = tuple(W.shape)
        self.data = torch.empty_like(W)
        _check(lib.ncf_attn_tail_pack_weight(_ptr(W), int(W.shape[0]), int(W.shape[1]), _ptr(self.data), _stream(W)))

    def is_contiguous(self):
        return True


def attn_tail(cand_emb: torch.Tensor, user, ubias: Optional[torch.Tensor], W1, b1, W2, b2, w3, b3: float) -> torch.Tensor:
    """ncf_attn_tail: merge of the attention partials (``user`` an AttnPartials; ``ubias`` = UserEmbeddings' bias) or finished user
    embeddings (``user`` a (B, UE) tensor, ``ubias`` None), cat(candidate_emb, user_emb), MLP -> (B, 1).  W1 / W2: both tensors in
    the reference's row-major layout, or both PackedTailWeight (the faster form, bit-identical)."""
    lib = load_library()
    _dev(cand_emb, "cand_emb")
    B, EA, ldc = _rows2d(cand_emb, "cand_emb")
    packed = isinstance(W1, PackedTailWeight)
    if packed != isinstance(W2, PackedTailWeight):
        raise TypeError("attn_tail: W1 and W2 must both be packed or both be plain tensors")
    N1, N2 = int(W1.shape[0]), int(W2.shape[0])
    out = torch.empty((B, 1), dtype=torch.float32, device=cand_emb.device)
    if isinstance(user, AttnPartials):
        part, ns, uptr, ldu, UE = user.ws, user.nsplit, None, 0, user.Fdim
    else:
        _, UE, ldu = _rows2d(user, "user_emb")
        part, ns, uptr = None, 1, user
    if W1.shape[1] != EA + UE or W2.shape[1] != N1 or w3.numel() != N2 or not (W1.is_contiguous() and W2.is_contiguous() and w3.is_contiguous()):
        raise ValueError("attn_tail: MLP weights do not match cat(candidate_emb, user_emb)")
    w1p, w2p = (W1.data, W2.data) if packed else (W1, W2)
    _check(lib.ncf_attn_tail(_ptr(cand_emb), ldc, EA, _ptr(part), ns, _ptr(uptr), ldu, UE, _ptr(ubias), _ptr(w1p), _ptr(b1), N1, _ptr(w2p), _ptr(b2), N2,
                             _ptr(w3), float(b3), 1 if packed else 0, _ptr(out), B, _stream(cand_emb)))
    return out


def attn_split_supported(mode: int, A: int, Fdim: int, pairs_per_wg: int) -> bool:
    return bool(load_library().ncf_attn_split_supported(int(mode), int(A), int(Fdim), int(pairs_per_wg)))


def default_attn_nsplit(B: int, n_rows: int, nnz: int, pairs_per_wg: int) -> int:
    """Slices of a rated set for the entry-split attention kernel, from sizes the host already holds (no device read): enough
    (group, slice) workgroups to give every CU two, at most one slice per 64-entry tile of an average row, at most 8."""
    if B <= 0 or n_rows <= 0:
        return 1
    groups = (B + pairs_per_wg - 1) // pairs_per_wg + min(n_rows, B) // 2          # between the bound and its half
    tiles = max(1, (nnz // max(n_rows, 1) + 63) // 64)
    want = (2 * num_cus() + groups - 1) // groups
    return int(max(1, min(want, tiles, 8)))


def num_cus() -> int:
    return 256


def attn_forward_grouped(mode: int, pc: torch.Tensor, pr: torch.Tensor, w1: Optional[torch.Tensor], b1: float,
                         rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, pair_row: torch.Tensor,
                         feat: torch.Tensor, out_bias: Optional[torch.Tensor] = None, pairs_per_wg: Optional[int] = None,
                         grouping=None, return_weights: bool = False, nsplit: Optional[int] = None, nnz_hint: Optional[int] = None,
                         leave_partials: bool = False):
    """LDS-tiled attention for pairs that share rated sets: CSR row ``pair_row[b]`` is pair b's set.  Returns out_feat
    (B, Fdim), or (out_feat, weights) with ``return_weights``: the attention weights in the layout of the expanded
    per-pair CSR (``SparseRatings.expanded()``).  ``grouping`` = (group_pairs(pair_row, R, ppw), ppw) computed earlier
    for this batch skips the sort.  Where ncf_attn_split_supported() holds (and no weights are asked for) the call takes the
    entry-split form (``nsplit`` slices of each rated set; default from the batch's sizes; 1 = one workgroup per group)."""
    lib = load_library()
    head, csr, ft, (B, I, A, Fdim) = _attn_operands(mode, pc, pr, w1, (rowptr, col, val), feat)
    if pair_row.numel() != B:
        raise ValueError("pair_row must name one CSR row per pair")
    R = rowptr.numel() - 1
    if grouping is not None:
        grp, pairs_per_wg = grouping
    else:
        if pairs_per_wg is None:
            pairs_per_wg = default_pairs_per_wg(B)
        grp = group_pairs(pair_row.to(torch.int64).contiguous(), R, pairs_per_wg)
    grp_ptr, pair_ids, wg_ptr = grp
    out = torch.empty((B, Fdim), dtype=torch.float32, device=pc.device)
    wg_row = getattr(grp, "wg_row", None)
    if (not return_weights and get_option("attn_grouped_kernel") == 0
            and lib.ncf_attn_split_supported(mode, A, Fdim, int(pairs_per_wg)) and I > 0):
        # entry-split form (round 3): (group of pairs) x (slice of the rated set) workgroups + a merge of the softmax partials
        ns = int(nsplit) if nsplit is not None else default_attn_nsplit(B, R, col.numel() if nnz_hint is None else int(nnz_hint), int(pairs_per_wg))
        nbytes = lib.ncf_attn_split_workspace_bytes(B, Fdim, ns)
        ws = _workspace(nbytes, pc.device) if ns > 1 else None
        _check(lib.ncf_attn_forward_split(*head, float(b1), *csr, R, I, _ptr(grp_ptr), _ptr(pair_ids), _ptr(wg_ptr), _ptr(wg_row), B,
                                          int(pairs_per_wg), *ft, _ptr(out_bias), _ptr(out), out.stride(0),
                                          ns, 0 if (leave_partials and ns > 1) else 1, _ptr(ws), nbytes, _stream(pc)))
        if leave_partials and ns > 1:
            return AttnPartials(ws, ns, Fdim, B)
        return out
    wts = wts_off = None
    if return_weights:
        lens = (rowptr[1:] - rowptr[:-1])[pair_row.to(torch.int64)]
        wts_off = (torch.cumsum(lens, 0) - lens).contiguous()
        # expanded nnz without a host sync is not available: size by the upper bound B * (longest row) would be wasteful,
        # so this one size is read back (return_weights is the explanation / plotting path, not the scoring loop)
        wts = torch.empty(max(int(lens.sum().item()), 1), dtype=torch.float32, device=pc.device)
    _check(lib.ncf_attn_forward_grouped(*head, float(b1), *csr, R, I, _ptr(grp_ptr), _ptr(pair_ids), _ptr(wg_ptr), B, int(pairs_per_wg),
                                        *ft, _ptr(out_bias), _ptr(out), out.stride(0), _ptr(wts), _ptr(wts_off), _stream(pc)))
    return (out, wts) if return_weights else out


def attn_logits(mode: int, pc: torch.Tensor, pr: torch.Tensor, w1: Optional[torch.Tensor], b1: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The logit table of a catalogue (ncf_attn_logits): ST (I_r, I_c) fp32, ST[e, i] = the attention logit of candidate i (row of
    ``pc``) against rated item e (row of ``pr``); modes and operands as ``attn_forward``.  One launch on the current stream."""
    lib = load_library()
    (_, ppc, ldpc, ppr, ldpr, A, pw1), _, _, (Ic, Ir, _, _) = _attn_operands(mode, pc, pr, w1)
    if out is None:
        out = torch.empty((Ir, Ic), dtype=torch.float32, device=pc.device)
    Ir2, Ic2, ldst = _rows2d(out, "out")
    if (Ir2, Ic2) != (Ir, Ic) or out.dtype != torch.float32:
        raise ValueError(f"out must be ({Ir}, {Ic}) fp32")
    # this entry takes each table's rows beside its pointer, so the shared head is taken apart
    _check(lib.ncf_attn_logits(int(mode), ppc, ldpc, Ic, ppr, ldpr, Ir, A, pw1, float(b1), _ptr(out), ldst, _stream(pc)))
    return out


def attn_cross_supported(Fdim: int) -> bool:
    """Widths ``attn_cross`` takes (ncf_attn_cross_supported: Fdim % 32 == 0, 32 <= Fdim <= 256).  Host only."""
    return load_library().ncf_attn_cross_supported(int(Fdim)) == 1


def attn_cross_plan(Fdim: int, U: int = 1, I: int = 1):
    """(nb, entry_tile, LDS bytes, grid_x) of the launch ``attn_cross`` would make: attn_cross_kernel<nb, entry_tile>.  Host only;
    raises NativeError where the call would refuse."""
    return _query(load_library().ncf_attn_cross_plan, (int(Fdim), int(U), int(I)), (_c_int, _c_int, _c_i64, _c_i64))


def attn_cross(ST: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, user_rows: torch.Tensor,
               feat: torch.Tensor, out_bias: Optional[torch.Tensor] = None, cand_ids: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of the listed users against the ranked list, from the logit table (ncf_attn_cross): (U * I, Fdim), row u * I + j =
    the user_emb of (user_rows[u], column j) — column j is table column ``cand_ids[j]``, or j without ``cand_ids`` (I = I_c).
    ``rowptr / col / val``: the users' CSR (col = rows of ST and of feat).  An out-of-range user row or candidate id raises at the
    next check_oob().  One launch on the current stream; nothing synchronises."""
    lib = load_library()
    _dev(ST, "ST")
    Ir, Ic, ldst = _rows2d(ST, "ST")
    Ir2, Fdim, ldf = _rows2d(feat, "feat")
    if Ir != Ir2:
        raise ValueError("ST and feat disagree on the number of rated items")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float32:
        raise TypeError("CSR must be (int64 rowptr, int32 col, fp32 val)")
    user_rows, cand_ids = _idx(user_rows), _idx(cand_ids)
    U = user_rows.numel()
    I = Ic if cand_ids is None else cand_ids.numel()
    if out is None:
        out = torch.empty((U * I, Fdim), dtype=torch.float32, device=ST.device)
    rows, F2, ldo = _rows2d(out, "out")
    if rows != U * I or F2 != Fdim or out.dtype != torch.float32:
        raise ValueError(f"out must be ({U * I}, {Fdim}) fp32")
    _check(lib.ncf_attn_cross(_ptr(ST), ldst, Ir, Ic, _ptr(rowptr), _ptr(col), _ptr(val), rowptr.numel() - 1, _ptr(user_rows), U,
                              _ptr(cand_ids), I, _ptr(feat), ldf, Fdim, _ptr(out_bias), _ptr(out), ldo, _ptr(_oob_flag(ST.device)),
                              _stream(ST)))
    return out


ATTN_EXPLAIN_MAX_REASONS = 64   # include/ncf_abi.h ncf_attn_explain_max_reasons


def attn_explain(ST: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, user_rows: torch.Tensor,
                 items: torch.Tensor, thr: torch.Tensor, max_reasons: int, out=None):
    """The reasons of (user, winner) pairs from the logit table (ncf_attn_explain): ``(col (U, k, E) int32, w (U, k, E) fp32,
    val (U, k, E) fp32, cnt (U, k) int32)`` with E = ``max_reasons`` — per pair the entries of the user's row whose attention weight
    towards table column ``items[u, s]`` exceeds ``thr[u]``, in descending weight (ties: the entry stored earlier), ``cnt`` uncapped,
    slots past ``min(cnt, E)`` as ``(-1, 0, 0)``.  ``ST / rowptr / col / val / user_rows`` as ``attn_cross`` takes them; ``items``
    (U, k) int64, -1 = an empty slot; ``thr`` (U,) fp32.  ``out``: the four tensors preallocated (contiguous).  An out-of-range user
    row or item raises at the next check_oob().  Every shape and dtype check comes before the first device use; one launch on the
    current stream; nothing synchronises."""
    E = int(max_reasons)
    if not 1 <= E <= ATTN_EXPLAIN_MAX_REASONS:
        raise ValueError(f"max_reasons = {max_reasons} is outside 1 .. {ATTN_EXPLAIN_MAX_REASONS}")
    Ir, Ic, ldst = _rows2d(ST, "ST")
    if ST.dtype != torch.float32:
        raise TypeError("ST must be fp32")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float32:
        raise TypeError("CSR must be (int64 rowptr, int32 col, fp32 val)")
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.shape != col.shape:
        raise ValueError("CSR must be 1-D (rowptr (rows + 1,), col (nnz,), val (nnz,))")
    user_rows = _idx(user_rows)
    U = user_rows.numel()
    if items.dtype != torch.int64 or items.dim() != 2 or items.shape[0] != U or not items.is_contiguous():
        raise ValueError(f"items must be a contiguous ({U}, k) int64 tensor")
    if thr.dtype != torch.float32 or thr.dim() != 1 or thr.numel() != U or not thr.is_contiguous():
        raise ValueError(f"thr must be a contiguous ({U},) fp32 tensor")
    k = items.shape[1]
    shapes = ((U, k, E), (U, k, E), (U, k, E), (U, k))
    dtypes = (torch.int32, torch.float32, torch.float32, torch.int32)
    if out is not None:
        if len(out) != 4 or any(tuple(o.shape) != s or o.dtype != d or not o.is_contiguous() for o, s, d in zip(out, shapes, dtypes)):
            raise ValueError(f"out must be contiguous (col {shapes[0]} int32, w fp32, val fp32, cnt {shapes[3]} int32)")
    named = [(ST, "ST"), (rowptr, "rowptr"), (col, "col"), (val, "val"), (user_rows, "user_rows"), (items, "items"), (thr, "thr")]
    for t, what in named + [(o, "out") for o in out or ()]:
        _dev(t, what)
    lib = load_library()
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=ST.device) for s, d in zip(shapes, dtypes))
    rc, rw, rv, cnt = out
    _check(lib.ncf_attn_explain(_ptr(ST), ldst, Ir, Ic, _ptr(rowptr), _ptr(col), _ptr(val), rowptr.numel() - 1, _ptr(user_rows), U,
                                _ptr(items), k, _ptr(thr), E, _ptr(rc), _ptr(rw), _ptr(rv), _ptr(cnt), _ptr(_oob_flag(ST.device)),
                                _stream(ST)))
    return rc, rw, rv, cnt


ATTN_STATS_SLAB = 512   # csrc/attn_stats.hip kStSlab: rated columns owned by one wave of the accumulation kernel


def attn_stats(ST: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, user_rows: torch.Tensor, cands: torch.Tensor,
               sum: torch.Tensor, count: torch.Tensor):
    """Item-item attention statistics of S samples from the logit table (ncf_attn_stats, the contract in include/ncf_abi.h), added
    IN PLACE to ``sum`` (I_c, I_r) float64 and ``count`` (I_c, I_r) int64 (row strides allowed): for sample s and every valid entry e
    of row ``user_rows[s]``, ``sum[cands[s], col_e] +=`` the fp32 attention weight of col_e towards ``cands[s]`` and ``count[...] += 1``.
    ``ST / rowptr / col`` as ``attn_explain`` takes them; ``user_rows`` and ``cands`` (S,) int64.  The additions into a cell happen
    in ascending sample index from the value already there: equal inputs give equal bits, and a file fed in consecutive pieces gives
    the bits of one call.  Valid columns within a row must be distinct.  The per-candidate sample lists are built here on the
    device (a stable sort of the candidates, ``searchsorted`` for the bucket offsets: neither reads a size on the host).  An
    out-of-range user row or candidate adds nothing and raises at the next check_oob().  Every shape and dtype check comes before the
    first device use; nothing synchronises.  Returns ``(sum, count)``."""
    Ir, Ic, ldst = _rows2d(ST, "ST")
    if ST.dtype != torch.float32:
        raise TypeError("ST must be fp32")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32:
        raise TypeError("CSR must be (int64 rowptr, int32 col)")
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or not rowptr.is_contiguous() or not col.is_contiguous():
        raise ValueError("CSR must be contiguous 1-D (rowptr (rows + 1,), col (nnz,))")
    user_rows, cands = _idx(user_rows), _idx(cands)
    S = user_rows.numel()
    if cands.numel() != S:
        raise ValueError(f"cands has {cands.numel()} entries for {S} user rows")
    if sum.dtype != torch.float64 or count.dtype != torch.int64:
        raise TypeError("sum must be float64 and count int64")
    for t, what in ((sum, "sum"), (count, "count")):
        if tuple(_rows2d(t, what)[:2]) != (Ic, Ir):
            raise ValueError(f"{what} must be ({Ic}, {Ir}): one row per candidate, one column per rated item")
    for t, what in ((ST, "ST"), (rowptr, "rowptr"), (col, "col"), (user_rows, "user_rows"), (cands, "cands"), (sum, "sum"), (count, "count")):
        _dev(t, what)
    lib = load_library()
    if S == 0:
        return sum, count
    key = torch.where((cands >= 0) & (cands < Ic), cands, torch.full_like(cands, Ic))      # out of range: after every bucket
    skey, order = torch.sort(key, stable=True)                                              # within a bucket: ascending sample index
    cand_rowptr = torch.searchsorted(skey, torch.arange(Ic + 1, dtype=torch.int64, device=ST.device))
    nbytes = lib.ncf_attn_stats_workspace_bytes(S)
    ws = _workspace(nbytes, ST.device)
    _check(lib.ncf_attn_stats(_ptr(ST), ldst, Ir, Ic, _ptr(rowptr), _ptr(col), rowptr.numel() - 1, _ptr(user_rows), _ptr(cands), S,
                              _ptr(order), _ptr(cand_rowptr), _ptr(sum), sum.stride(0), _ptr(count), count.stride(0),
                              _ptr(_oob_flag(ST.device)), _ptr(ws), nbytes, _stream(ST)))
    return sum, count


def l2_normalize_rows(x: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    _dev(x, "x")
    R, E, ld = _rows2d(x, "x")
    out = torch.empty((R, E), dtype=torch.float32, device=x.device)
    _check(lib.ncf_l2_normalize_rows(_ptr(x), ld, R, E, _ptr(out), out.stride(0), _stream(x)))
    return out


def user_profiles(rowptr: torch.Tensor, col: torch.Tensor, rating: torch.Tensor, avg: torch.Tensor, features: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fixed user profiles (ncf_user_profiles, the contract in include/ncf_abi.h): out[u] = the float64 mean over user u's ratings, in
    order, of (rating - avg[u]) * features[col], rounded to fp32; an empty row gives zeros.  ``rowptr`` (U + 1,) int64, ``col`` int32 and
    ``rating`` fp32 of one entry per rating, ``avg`` (U,) float64, ``features`` (I, F) fp32 rows (a column slice is fine).  A column
    outside [0, I) sets the sticky out-of-range flag (check_oob) and adds nothing.  Shapes, dtypes and layout are checked before the
    device is."""
    who = "user_profiles"
    _vec1d(who, avg, "avg", torch.float64)
    U = avg.numel()
    _vec1d(who, rowptr, "rowptr", torch.int64, U + 1)
    _vec1d(who, col, "col", torch.int32)
    _vec1d(who, rating, "rating", torch.float32, col.numel())
    _table_f32(who, features, "features", 0)
    (I, F), ldf = features.shape, features.stride(0)
    out = _out2d(who, out, U, F, features, ((rowptr, "rowptr"), (col, "col"), (rating, "rating"), (avg, "avg"), (features, "features")))
    lib = load_library()
    _check(lib.ncf_user_profiles(_ptr(rowptr), _ptr(col), _ptr(rating), col.numel(), _ptr(avg), U, _ptr(features), I, ldf, F, _ptr(out),
                                 out.stride(0), _ptr(_oob_flag(features.device)), _stream(features)))
    return out


KMF_MAX_FACTORS, KMF_MAX_BLOCKS = 256, 1024       # csrc/kmf.hip


def kmf_flag(device) -> torch.Tensor:
    """The sticky int32 flag word of the KernelMF kernels on ``device`` (bits KMF_FLAG_*)."""
    return _flag("kmf", device)


def check_kmf(device, flag: Optional[torch.Tensor] = None):
    """Synchronising check of the KernelMF flag word: raises IndexError, and clears it, when a kernel met an id outside its table, a
    sample filed in the wrong block or a broken block / row pointer (each such sample or block was skipped)."""
    _check_flag("kmf", device, flag)


def _kmf_factors(who, PU, QI, F):
    """F of a KernelMF call, whose two tables hold F factors and the bias in a row."""
    F = int(F)
    if F < 1:
        raise ValueError(f"{who}: F = {F} is not at least one factor")
    _table_f32(who, PU, "PU", F + 1)
    _table_f32(who, QI, "QI", F + 1)
    return F


def kmf_epoch(PU: torch.Tensor, QI: torch.Tensor, F: int, user: torch.Tensor, item: torch.Tensor, rating: torch.Tensor,
              block_ptr: torch.Tensor, user_block: torch.Tensor, item_block: torch.Tensor, mu: float, lr: float, reg: float,
              n_epochs: int = 1, sse: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``n_epochs`` epochs of stratified SGD over a prepared plan, in place on the KernelMF tables (ncf_kmf_epoch, THE CONTRACT in
    include/ncf_abi.h).  ``PU`` (U, >= F + 1) and ``QI`` (I, >= F + 1) fp32 rows: F factors, then the bias.  ``user`` / ``item`` int32
    and ``rating`` fp32 are the samples in stratum-major block order, ``block_ptr`` (W * W + 1,) int64, ``user_block`` (U,) and
    ``item_block`` (I,) int32.  Returns the (n_epochs, W) float64 partial sums of squared errors (``sse`` when given: ADDED to).  What
    the kernel refuses sets ``flag`` (default: the device's word, check_kmf).  Shapes, dtypes and layout are checked before the device
    is."""
    who = "kmf_epoch"
    F = _kmf_factors(who, PU, QI, F)
    U, I = PU.shape[0], QI.shape[0]
    _vec1d(who, user, "user", torch.int32)
    n = user.numel()
    _vec1d(who, item, "item", torch.int32, n)
    _vec1d(who, rating, "rating", torch.float32, n)
    _vec1d(who, block_ptr, "block_ptr", torch.int64)
    W = int(round((block_ptr.numel() - 1) ** 0.5)) if block_ptr.numel() > 1 else 0
    if W < 1 or W * W + 1 != block_ptr.numel() or W > KMF_MAX_BLOCKS:
        raise ValueError(f"{who}: block_ptr has {block_ptr.numel()} entries, not W * W + 1 for a W in 1 .. {KMF_MAX_BLOCKS}")
    _vec1d(who, user_block, "user_block", torch.int32, U)
    _vec1d(who, item_block, "item_block", torch.int32, I)
    n_epochs = int(n_epochs)
    if n_epochs < 0:
        raise ValueError(f"{who}: n_epochs = {n_epochs}")
    _out1d(who, sse, "sse", torch.float64, n_epochs * W)
    _out1d(who, flag, "flag", torch.int32, 1)
    _dev_all((PU, "PU"), (QI, "QI"), (user, "user"), (item, "item"), (rating, "rating"), (block_ptr, "block_ptr"),
             (user_block, "user_block"), (item_block, "item_block"), (sse, "sse"), (flag, "flag"))
    lib = load_library()
    if sse is None:
        sse = torch.zeros((n_epochs, W), dtype=torch.float64, device=PU.device)
    if flag is None:
        flag = kmf_flag(PU.device)
    if n and n_epochs and U and I:
        _check(lib.ncf_kmf_epoch(_ptr(PU), PU.stride(0), U, _ptr(QI), QI.stride(0), I, F, _ptr(user), _ptr(item), _ptr(rating), n,
                                 _ptr(block_ptr), _ptr(user_block), _ptr(item_block), W, float(mu), float(lr), float(reg), n_epochs,
                                 _ptr(sse), _ptr(flag), _stream(PU)))
    return sse


def kmf_fold_users(PU: torch.Tensor, QI: torch.Tensor, F: int, users: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor,
                   rating: torch.Tensor, mu: float, lr: float, reg: float, n_epochs: int = 1, sse: Optional[torch.Tensor] = None,
                   flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fold-in of users against the fixed item table (ncf_kmf_fold_users): ``n_epochs`` passes of the contract's user-side update
    over row k of the CSR (``rowptr`` (n_users + 1,) int64, ``col`` int32 item positions, ``rating`` fp32) for user ``users[k]`` (int32,
    no user twice), in place on ``PU``; ``QI`` is only read.  Returns the (n_epochs, n_users) float64 sums of squared errors (``sse``
    when given: overwritten).  Checked before the device is, as kmf_epoch."""
    who = "kmf_fold_users"
    F = _kmf_factors(who, PU, QI, F)
    U, I = PU.shape[0], QI.shape[0]
    _vec1d(who, users, "users", torch.int32)
    nu = users.numel()
    _, nnz = _csr(who, rowptr, col, rating, ("rowptr", "col", "rating"), nu)
    n_epochs = int(n_epochs)
    if n_epochs < 0:
        raise ValueError(f"{who}: n_epochs = {n_epochs}")
    _out1d(who, sse, "sse", torch.float64, n_epochs * nu)
    _out1d(who, flag, "flag", torch.int32, 1)
    _dev_all((PU, "PU"), (QI, "QI"), (users, "users"), (rowptr, "rowptr"), (col, "col"), (rating, "rating"), (sse, "sse"), (flag, "flag"))
    lib = load_library()
    if sse is None:
        sse = torch.zeros((n_epochs, nu), dtype=torch.float64, device=PU.device)
    if flag is None:
        flag = kmf_flag(PU.device)
    if nu and n_epochs:
        _check(lib.ncf_kmf_fold_users(_ptr(PU), PU.stride(0), U, _ptr(QI), QI.stride(0), I, F, _ptr(users), nu, _ptr(rowptr), _ptr(col),
                                      _ptr(rating), nnz, float(mu), float(lr), float(reg), n_epochs, _ptr(sse), _ptr(flag), _stream(PU)))
    return sse


KNN_MAX_N, KNN_MAX_TILE, KNN_MAX_STAGE, KNN_MAX_ROWS = 256, 8192, 8192, 65535       # csrc/knn.hip


def knn_flag(device) -> torch.Tensor:
    """The sticky int32 word of ncf_knn_sim_rows on ``device``: set by a row whose columns do not strictly ascend."""
    return _flag("knn", device)


def check_knn(device, flag: Optional[torch.Tensor] = None):
    """Synchronising check of the ItemKNN flag word: raises ValueError, and clears it, when ncf_knn_sim_rows walked a row of the user
    CSR whose columns do not strictly ascend (a duplicate rating or an unsorted row; the similarities of such a fit are unspecified)."""
    _check_flag("knn", device, flag)


def _knn_range(who, item_range, I):
    i0, i1 = (0, I) if item_range is None else (int(item_range[0]), int(item_range[1]))
    if not 0 <= i0 <= i1 <= I:
        raise ValueError(f"{who}: items [{i0}, {i1}) outside [0, {I})")
    return i0, i1


def _knn_table(who, nb_pos, nb_sim, nb_cnt):
    if not torch.is_tensor(nb_pos) or nb_pos.dtype != torch.int32 or nb_pos.dim() != 2 or not nb_pos.is_contiguous():
        raise ValueError(f"{who}: nb_pos must be a contiguous (I, N) int32 tensor")
    I, N = nb_pos.shape
    if not torch.is_tensor(nb_sim) or nb_sim.dtype != torch.float32 or tuple(nb_sim.shape) != (I, N) or not nb_sim.is_contiguous():
        raise ValueError(f"{who}: nb_sim must be a contiguous ({I}, {N}) float32 tensor")
    _vec1d(who, nb_cnt, "nb_cnt", torch.int32, I)
    if not 1 <= N <= KNN_MAX_N:
        raise ValueError(f"{who}: N = {N} neighbours per item is outside 1 .. {KNN_MAX_N}")
    return I, N


def knn_item_sq(colptr: torch.Tensor, tval: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(I,) fp32 squared norms of the item columns of a transposed ratings CSR (ncf_knn_item_sq, THE CONTRACT in include/ncf_abi.h):
    ``colptr`` (I + 1,) int64, ``tval`` fp32.  Checked before the device is; one launch on the current stream."""
    who = "knn_item_sq"
    _vec1d(who, colptr, "colptr", torch.int64)
    if colptr.numel() < 1:
        raise ValueError(f"{who}: colptr is empty")
    _vec1d(who, tval, "tval", torch.float32)
    I = colptr.numel() - 1
    _out1d(who, out, "out", torch.float32, I)
    _dev_all((colptr, "colptr"), (tval, "tval"), (out, "out"))
    lib = load_library()
    if out is None:
        out = torch.empty(I, dtype=torch.float32, device=colptr.device)
    _check(lib.ncf_knn_item_sq(_ptr(colptr), _ptr(tval), tval.numel(), I, _ptr(out), _ptr(_oob_flag(colptr.device)), _stream(colptr)))
    return out


def knn_sim_rows(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, colptr: torch.Tensor, row: torch.Tensor, tval: torch.Tensor,
                 sq: torch.Tensor, item_range=None, min_support: int = 1, shrink: float = 0.0, col_tile: int = 0,
                 out: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The similarity rows of the items ``item_range`` = (i0, i1) (default: all) as a dense (i1 - i0, I) fp32 tensor
    (ncf_knn_sim_rows, THE CONTRACT in include/ncf_abi.h).  ``rowptr`` / ``col`` / ``val``: the user CSR (int64 / int32 strictly
    ascending in a row / fp32); ``colptr`` / ``row`` / ``tval``: its transpose; ``sq`` (I,) fp32 from knn_item_sq.  ``col_tile``: 0 =
    choose, else a multiple of 64.  An id outside its range raises at the next check_oob(), a non-ascending row at check_knn()
    (``flag``: another word than the device's).  Checked before the device is; one launch on the current stream."""
    who = "knn_sim_rows"
    U, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    I, nnzT = _csr(who, colptr, row, tval, ("colptr", "row", "tval"))
    _vec1d(who, sq, "sq", torch.float32, I)
    i0, i1 = _knn_range(who, item_range, I)
    if i1 - i0 > KNN_MAX_ROWS:
        raise ValueError(f"{who}: {i1 - i0} items in one call (at most {KNN_MAX_ROWS})")
    min_support = _int_in(who, min_support, "min_support", 1, 2 ** 31 - 1)
    shrink = _finite(who, shrink, "shrink", 0.0)
    col_tile = _int_in(who, col_tile, "col_tile", 0, KNN_MAX_TILE)
    if col_tile % 64:
        raise ValueError(f"{who}: col_tile = {col_tile} is not a multiple of 64")
    _out1d(who, flag, "flag", torch.int32, 1)
    out = _out2d(who, out, i1 - i0, I, rowptr, ((rowptr, "rowptr"), (col, "col"), (val, "val"), (colptr, "colptr"), (row, "row"), (tval, "tval"),
                                                (sq, "sq"), (flag, "flag")))
    lib = load_library()
    dev = rowptr.device
    if flag is None:
        flag = knn_flag(dev)
    if i1 > i0 and I:
        _check(lib.ncf_knn_sim_rows(_ptr(rowptr), _ptr(col), _ptr(val), nnz, U, _ptr(colptr), _ptr(row), _ptr(tval), nnzT, I, _ptr(sq), i0, i1,
                                    min_support, shrink, col_tile, _ptr(out), max(out.stride(0), I), _ptr(_oob_flag(dev)), _ptr(flag),
                                    _stream(rowptr)))
    return out


def knn_scores(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, users: torch.Tensor, nb_pos: torch.Tensor, nb_sim: torch.Tensor,
               nb_cnt: torch.Tensor, item_range=None, weighted_average: bool = True, fill: float = 0.0, stage_cap: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, i1 - i0) fp32 ItemKNN scores of the rows ``users`` (int64) of a ratings CSR against the items ``item_range`` (default: all)
    of a neighbour table ``nb_pos`` (I, N) int32 / ``nb_sim`` (I, N) fp32 / ``nb_cnt`` (I,) int32 (ncf_knn_scores, THE CONTRACT in
    include/ncf_abi.h).  The CSR need not be the fitted one.  ``stage_cap``: rows of at most that many entries are staged in LDS
    (0 = the default); the bits do not depend on it.  A row outside the CSR scores as an empty one and raises at the next
    check_oob().  Checked before the device is; one launch on the current stream."""
    who = "knn_scores"
    R, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    _vec1d(who, users, "users", torch.int64)
    B = users.numel()
    if B > KNN_MAX_ROWS:
        raise ValueError(f"{who}: {B} users in one call (at most {KNN_MAX_ROWS})")
    I, N = _knn_table(who, nb_pos, nb_sim, nb_cnt)
    i0, i1 = _knn_range(who, item_range, I)
    fill = _finite(who, fill, "fill")
    stage_cap = _int_in(who, stage_cap, "stage_cap", 0, KNN_MAX_STAGE)
    out = _out2d(who, out, B, i1 - i0, rowptr, ((rowptr, "rowptr"), (col, "col"), (val, "val"), (users, "users"), (nb_pos, "nb_pos"),
                                                (nb_sim, "nb_sim"), (nb_cnt, "nb_cnt")))
    lib = load_library()
    dev = rowptr.device
    if B and i1 > i0:
        _check(lib.ncf_knn_scores(_ptr(rowptr), _ptr(col), _ptr(val), nnz, R, _ptr(users), B, _ptr(nb_pos), _ptr(nb_sim), _ptr(nb_cnt), I, N,
                                  i0, i1, 1 if weighted_average else 0, fill, stage_cap, _ptr(out), max(out.stride(0), i1 - i0),
                                  _ptr(_oob_flag(dev)), _stream(rowptr)))
    return out


def knn_predict(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, users: torch.Tensor, items: torch.Tensor, nb_pos: torch.Tensor,
                nb_sim: torch.Tensor, nb_cnt: torch.Tensor, weighted_average: bool = True, fill: float = 0.0) -> torch.Tensor:
    """(n,) fp32 ItemKNN scores of the pairs (``users[k]`` row of the CSR, ``items[k]``), both int64 (ncf_knn_predict): knn_scores'
    value of that user and item, bit for bit.  A row or an item outside its range scores as an empty row and raises at the next
    check_oob().  Checked before the device is; one launch on the current stream."""
    who = "knn_predict"
    R, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    _vec1d(who, users, "users", torch.int64)
    n = users.numel()
    _vec1d(who, items, "items", torch.int64, n)
    I, N = _knn_table(who, nb_pos, nb_sim, nb_cnt)
    fill = _finite(who, fill, "fill")
    _dev_all((rowptr, "rowptr"), (col, "col"), (val, "val"), (users, "users"), (items, "items"), (nb_pos, "nb_pos"), (nb_sim, "nb_sim"),
             (nb_cnt, "nb_cnt"))
    lib = load_library()
    dev = rowptr.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        _check(lib.ncf_knn_predict(_ptr(rowptr), _ptr(col), _ptr(val), nnz, R, _ptr(users), _ptr(items), n, _ptr(nb_pos), _ptr(nb_sim),
                                   _ptr(nb_cnt), I, N, 1 if weighted_average else 0, fill, _ptr(out), _ptr(_oob_flag(dev)), _stream(rowptr)))
    return out


EASE_BLOCK, EASE_MAX_ITEMS, EASE_MAX_ROWS, EASE_MAX_STAGE = 128, 65535, 65535, 8192       # include/ncf_abi.h NCF_EASE_BLOCK, csrc/ease.hip


def ease_flag(device) -> torch.Tensor:
    """The sticky int32 flag word of the EASE kernels on ``device`` (bits EASE_FLAG_*)."""
    return _flag("ease", device)


def check_ease(device, flag: Optional[torch.Tensor] = None):
    """Synchronising check of the EASE flag word: raises ValueError, and clears it, when ncf_ease_gram walked a row of the user CSR
    whose columns do not strictly ascend or ncf_ease_invert met a pivot that is not positive and finite (its output is zeros)."""
    _check_flag("ease", device, flag)


def _ease_matrix(who, M, what, square=True):
    """A 2-D float32 matrix with unit inner stride, square unless told otherwise, at most EASE_MAX_ITEMS wide; returns (rows, ld)."""
    _table_f32(who, M, what, 0)
    if square and M.shape[0] != M.shape[1]:
        raise ValueError(f"{who}: {what} must be square, got {tuple(M.shape)}")
    if M.shape[1] > EASE_MAX_ITEMS:
        raise ValueError(f"{who}: {M.shape[1]} items (at most {EASE_MAX_ITEMS})")
    return M.shape[0], max(M.stride(0), M.shape[1]) if M.shape[0] > 1 else M.shape[1]


def ease_gram(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, colptr: torch.Tensor, row: torch.Tensor, tval: torch.Tensor,
              item_range=None, out: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rows ``item_range`` = (i0, i1) (default: all) of the Gram matrix X^T X as a dense (i1 - i0, I) fp32 tensor (ncf_ease_gram,
    THE CONTRACT in include/ncf_abi.h): knn_sim_rows' arguments and walk, no float atomics, one fixed order, G == G^T bit for bit.  An
    id outside its range raises at the next check_oob(), a non-ascending row at check_ease() (``flag``: another word than the
    device's).  Checked before the device is; one launch on the current stream."""
    who = "ease_gram"
    U, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    I, nnzT = _csr(who, colptr, row, tval, ("colptr", "row", "tval"))
    if I > EASE_MAX_ITEMS:
        raise ValueError(f"{who}: {I} items (at most {EASE_MAX_ITEMS})")
    i0, i1 = _knn_range(who, item_range, I)
    _out1d(who, flag, "flag", torch.int32, 1)
    out = _out2d(who, out, i1 - i0, I, rowptr, ((rowptr, "rowptr"), (col, "col"), (val, "val"), (colptr, "colptr"), (row, "row"), (tval, "tval"),
                                                (flag, "flag")))
    lib = load_library()
    dev = rowptr.device
    if flag is None:
        flag = ease_flag(dev)
    if i1 > i0 and I:
        _check(lib.ncf_ease_gram(_ptr(rowptr), _ptr(col), _ptr(val), nnz, U, _ptr(colptr), _ptr(row), _ptr(tval), nnzT, I, i0, i1, _ptr(out),
                                 max(out.stride(0), I), _ptr(_oob_flag(dev)), _ptr(flag), _stream(rowptr)))
    return out


def ease_invert(A: torch.Tensor, lam: float, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adds ``lam`` to the diagonal of the square fp32 matrix ``A`` (unit inner stride, any row stride) and replaces it IN PLACE by its
    inverse (ncf_ease_invert, THE CONTRACT in include/ncf_abi.h): blocked Gauss-Jordan without pivoting, panels of EASE_BLOCK, every
    update a tiled fp32 MFMA GEMM; the same bits on every run.  ``A`` must be symmetric positive semi-definite: a pivot that is not
    positive and finite gives zeros and raises at check_ease() (``flag``: another word than the device's).  Returns ``A``.  Checked
    before the device is; 1 + 3 * ceil(N / EASE_BLOCK) launches on the current stream."""
    who = "ease_invert"
    N, lda = _ease_matrix(who, A, "A")
    lam = _finite(who, lam, "lam")
    if not lam > 0:
        raise ValueError(f"{who}: lam = {lam} is not > 0")
    _out1d(who, flag, "flag", torch.int32, 1)
    _dev_all((A, "A"), (flag, "flag"))
    lib = load_library()
    if N:
        nbytes = lib.ncf_ease_invert_workspace_bytes(N)
        ws = _workspace(nbytes, A.device)
        _check(lib.ncf_ease_invert(_ptr(A), N, lda, lam, _ptr(ws), nbytes, _ptr(ease_flag(A.device) if flag is None else flag), _stream(A)))
    return A


def ease_weights(P: torch.Tensor, diag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Replaces the square fp32 matrix ``P`` IN PLACE by the EASE weights W[i][j] = -(P[i][j] / P[j][j]), W[j][j] = +0.0
    (ncf_ease_weights): the correctly rounded division, bit for bit tests/ease_ref.py.  ``diag`` (N,) fp32 receives P's diagonal.
    Returns ``P``.  Checked before the device is; two launches on the current stream."""
    who = "ease_weights"
    N, ldp = _ease_matrix(who, P, "P")
    _out1d(who, diag, "diag", torch.float32, N)
    _dev_all((P, "P"), (diag, "diag"))
    lib = load_library()
    if N:
        if diag is None:
            diag = torch.empty(N, dtype=torch.float32, device=P.device)
        _check(lib.ncf_ease_weights(_ptr(P), N, ldp, _ptr(diag), _stream(P)))
    return P


def ease_scores(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, users: torch.Tensor, W: torch.Tensor, item_range=None,
                stage_cap: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, i1 - i0) fp32 EASE scores s = sum of val_e * W[col_e][j] of the rows ``users`` (int64) of a ratings CSR against the items
    ``item_range`` (default: all) of the (I, I) fp32 weights ``W`` (ncf_ease_scores, THE CONTRACT in include/ncf_abi.h).  The CSR need
    not be the fitted one.  ``stage_cap``: rows of at most that many entries are staged in LDS (0 = the default); the bits do not
    depend on it.  A row outside the CSR scores as an empty one, a column outside the items adds nothing; both raise at the next
    check_oob().  ``out``: a (B, >= i1 - i0) tensor to write into.  Checked before the device is; one launch on the current stream."""
    who = "ease_scores"
    R, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    _vec1d(who, users, "users", torch.int64)
    B = users.numel()
    if B > EASE_MAX_ROWS:
        raise ValueError(f"{who}: {B} users in one call (at most {EASE_MAX_ROWS})")
    I, ldw = _ease_matrix(who, W, "W")
    i0, i1 = _knn_range(who, item_range, I)
    stage_cap = _int_in(who, stage_cap, "stage_cap", 0, EASE_MAX_STAGE)
    out = _out2d(who, out, B, i1 - i0, rowptr, ((rowptr, "rowptr"), (col, "col"), (val, "val"), (users, "users"), (W, "W")), wider=True)
    lib = load_library()
    if B and i1 > i0:
        _check(lib.ncf_ease_scores(_ptr(rowptr), _ptr(col), _ptr(val), nnz, R, _ptr(users), B, _ptr(W), I, ldw, i0, i1, stage_cap, _ptr(out),
                                   max(out.stride(0), i1 - i0), _ptr(_oob_flag(rowptr.device)), _stream(rowptr)))
    return out


def ease_predict(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, users: torch.Tensor, items: torch.Tensor,
                 W: torch.Tensor) -> torch.Tensor:
    """(n,) fp32 EASE scores of the pairs (``users[k]`` row of the CSR, ``items[k]``), both int64 (ncf_ease_predict): ease_scores' value
    of that user and item, bit for bit.  A row or an item outside its range scores 0 and raises at the next check_oob().  Checked
    before the device is; one launch on the current stream."""
    who = "ease_predict"
    R, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    _vec1d(who, users, "users", torch.int64)
    n = users.numel()
    _vec1d(who, items, "items", torch.int64, n)
    I, ldw = _ease_matrix(who, W, "W")
    _dev_all((rowptr, "rowptr"), (col, "col"), (val, "val"), (users, "users"), (items, "items"), (W, "W"))
    lib = load_library()
    out = torch.empty(n, dtype=torch.float32, device=rowptr.device)
    if n:
        _check(lib.ncf_ease_predict(_ptr(rowptr), _ptr(col), _ptr(val), nnz, R, _ptr(users), _ptr(items), n, _ptr(W), I, ldw, _ptr(out),
                                    _ptr(_oob_flag(rowptr.device)), _stream(rowptr)))
    return out


SLIM_MAX_ITEMS = 32768       # include/ncf_abi.h NCF_SLIM_MAX_ITEMS


def slim_solve(G: torch.Tensor, l1: float, l2: float, cols: Optional[torch.Tensor] = None, positive: bool = True, warm: bool = False,
               max_sweeps: int = 100, tol: float = 1e-4, out: Optional[torch.Tensor] = None):
    """Columns ``cols`` (int32, default: all, in ascending order) of the SLIM weights of the square fp32 Gram matrix ``G`` by cyclic
    coordinate descent (ncf_slim_solve, THE CONTRACT in include/ncf_abi.h): column j minimises 1/2 w^T G w - G[j]^T w +
    1/2 l2 |w|^2 + l1 |w|_1 with w[j] = 0, and w >= 0 with ``positive``.  Returns ``(Wt, sweeps, steps, last)``: ``Wt`` (I, I) fp32
    whose ROW j is column j of W (``out``: a tensor to write into, any row stride; rows that are not listed keep what they hold, and
    are zeros in a tensor allocated here), and per listed column its sweeps (int32), its updates with delta != 0 (int32) and the
    largest |delta| of its last sweep (fp32: above ``tol`` the column met ``max_sweeps`` first).  ``warm``: start from the rows of
    ``out``.  One workgroup per listed column, started in list order; bit for bit tests/slim_ref.py.  A column outside the items
    raises at the next check_oob().  Checked before the device is; two launches on the current stream."""
    who = "slim_solve"
    I, ldg = _ease_matrix(who, G, "G")
    if I > SLIM_MAX_ITEMS:
        raise ValueError(f"{who}: {I} items (at most {SLIM_MAX_ITEMS})")
    l1, l2, tol = _finite(who, l1, "l1", 0.0), _finite(who, l2, "l2", 0.0), _finite(who, tol, "tol", 0.0)
    max_sweeps = _int_in(who, max_sweeps, "max_sweeps", 1, 2 ** 31 - 1)
    for v, what in ((positive, "positive"), (warm, "warm")):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {what} = {v!r} is not a bool")
    if cols is not None:
        _vec1d(who, cols, "cols", torch.int32)
    if warm and out is None:
        raise ValueError(f"{who}: a warm start reads its rows from out")
    given = out is not None
    out = _out2d(who, out, I, I, G, ((G, "G"), (cols, "cols")))
    lib = load_library()
    dev = G.device
    if cols is None:
        cols = torch.arange(I, dtype=torch.int32, device=dev)
    elif not given:
        out.zero_()
    n = cols.numel()
    sweeps = torch.empty(n, dtype=torch.int32, device=dev)
    steps = torch.empty(n, dtype=torch.int32, device=dev)
    last = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        _check(lib.ncf_slim_solve(_ptr(G), I, ldg, _ptr(cols), n, l1, l2, 1 if positive else 0, 1 if warm else 0, max_sweeps, tol, _ptr(out),
                                  max(out.stride(0), I) if I > 1 else max(I, 1), _ptr(sweeps), _ptr(steps), _ptr(last),
                                  _ptr(_oob_flag(dev)), _stream(G)))
    return out, sweeps, steps, last


ALS_MAX_FACTORS, ALS_GRAM_ROWS, ALS_SEG = 128, 256, 512       # include/ncf_abi.h NCF_ALS_*
ALS_BLOCK_BYTES = 256 << 20


def als_flag(device) -> torch.Tensor:
    """The sticky int32 flag word of ncf_als_solve_rows on ``device`` (bits ALS_FLAG_*)."""
    return _flag("als", device)


def check_als(device, flag: Optional[torch.Tensor] = None):
    """Synchronising check of the ImplicitALS flag word: raises, and clears it, when a half-sweep met a column outside the fixed
    table or a value that is negative or not finite (each such entry was skipped), a row outside the CSR or a broken pointer pair, a
    row whose columns do not strictly ascend or a pivot that is not positive (each such row was written as zeros).  IndexError when
    an id or a pointer was at fault, ValueError otherwise."""
    _check_flag("als", device, flag)


def _als_factors(who, T, F=None):
    """F of an ALS call (default: T's row) within 1 .. ALS_MAX_FACTORS, which the fp32 table ``T`` must hold in a row."""
    if F is not None:
        F = _int_in(who, F, "F", 1, ALS_MAX_FACTORS)
    _table_f32(who, T, "T", 1 if F is None else F)
    return _int_in(who, T.shape[1], "F", 1, ALS_MAX_FACTORS) if F is None else F


def als_gram(T: torch.Tensor, F: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(F, F) fp32 Gram matrix of the first ``F`` columns (default: all) of the (rows, >= F) fp32 table ``T`` (ncf_als_gram, THE
    CONTRACT in include/ncf_abi.h): chunks of 256 rows summed serially, the chunks added in ascending order, the upper triangle the
    mirror.  Checked before the device is; two launches on the current stream."""
    who = "als_gram"
    F = _als_factors(who, T, F)
    out = _out2d(who, out, F, F, T, ((T, "T"),), contiguous=True)
    lib = load_library()
    rows = T.shape[0]
    nbytes = lib.ncf_als_gram_workspace_bytes(rows, F)
    ws = _workspace(nbytes, T.device) if nbytes else None          # rows == 0: no chunk to write, and the entry takes a null pointer
    _check(lib.ncf_als_gram(_ptr(T), rows, max(T.stride(0), F), F, _ptr(out), _ptr(ws), nbytes, _stream(T)))
    return out


def als_plan(rowptr: torch.Tensor, rows: torch.Tensor, F: int, block_bytes: int = ALS_BLOCK_BYTES):
    """The plan of a half-sweep over the listed ``rows`` (int64) of a CSR with pointers ``rowptr``: a list of batches ``(k0, k1,
    seg_base, seg_row, n_slots)`` of consecutive listed rows whose segments beyond the first (rows longer than ALS_SEG entries) fit a
    scratch buffer of ``block_bytes``.  The bits of a half-sweep do not depend on the batches.  Reads the row lengths on the host (one
    synchronisation); a row outside the CSR or a broken pointer pair plans as a short row, which the kernel reports."""
    import numpy as np
    who = "als_plan"
    _vec1d(who, rowptr, "rowptr", torch.int64)
    _vec1d(who, rows, "rows", torch.int64)
    F = _int_in(who, F, "F", 1, ALS_MAX_FACTORS)
    block_bytes = _int_in(who, block_bytes, "block_bytes", 1, 2 ** 62)
    R, B = rowptr.numel() - 1, rows.numel()
    if R < 0:
        raise ValueError(f"{who}: rowptr is empty")
    cap = min(block_bytes // (4 * F * F), 2 ** 31 - 1)
    if B == 0 or R == 0:
        return [(0, B, None, None, 0)] if B else []
    inside = (rows >= 0) & (rows < R)
    r = rows.clamp(0, R - 1)
    beg, end = rowptr[r], rowptr[r + 1]
    n = torch.where(inside & (beg >= 0) & (end >= beg) & (end <= rowptr[-1].clamp_min(0)), end - beg, torch.zeros_like(beg))
    nseg = ((n + (ALS_SEG - 1)) // ALS_SEG).cpu().numpy()
    nl = np.where(nseg > 1, nseg, 0)
    if nl.max() > cap:
        raise ValueError(f"{who}: block_bytes = {block_bytes} holds {cap} segments of {F} x {F} floats; the longest row has {int(nl.max())}")
    cum = np.cumsum(nl)
    if cum[-1] == 0:
        return [(0, B, None, None, 0)]
    batches, k0, done = [], 0, 0
    while k0 < B:
        k1 = int(np.searchsorted(cum, done + cap, side="right"))          # the listed rows [k0, k1) hold at most cap segments
        part = nl[k0:k1]
        n_slots = int(part.sum())
        if n_slots:
            base = np.where(part > 0, cum[k0:k1] - part - done, -1).astype(np.int64)
            seg_row = np.repeat(np.arange(k1 - k0, dtype=np.int64), part)
            batches.append((k0, k1, torch.from_numpy(base).to(rows.device), torch.from_numpy(seg_row).to(rows.device), n_slots))
        else:
            batches.append((k0, k1, None, None, 0))
        k0, done = k1, int(cum[k1 - 1])
    return batches


def als_solve_rows(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, rows: torch.Tensor, T: torch.Tensor, G: torch.Tensor,
                   alpha: float, reg: float, out: Optional[torch.Tensor] = None, out_by_row: bool = False, plan=None,
                   block_bytes: int = ALS_BLOCK_BYTES, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ALS half-sweep (ncf_als_solve_rows, THE CONTRACT in include/ncf_abi.h): for each listed row (``rows`` int64) of the CSR
    ``rowptr`` int64 / ``col`` int32 strictly ascending in a row / ``val`` fp32 >= 0 over the rows of the fixed (n_t, >= F) fp32 table
    ``T``, x = (G + sum (alpha v) t t^T + reg I)^-1 sum (1 + alpha v) t by Cholesky.  ``G`` is the contiguous (F, F) Gram matrix
    (als_gram(T)), which also fixes F.  Returns the (B, F) rows, row k for ``rows[k]``; with ``out_by_row`` they are written to the rows
    ``rows[k]`` of ``out`` ((R, >= F); required then) and no other row of it is touched.  ``plan``: als_plan's batches for these rows
    (built here, with one synchronisation, when absent); ``block_bytes`` sizes the scratch buffer of the rows longer than one segment
    and does not change a bit.  What the kernel refuses sets ``flag`` (default: the device's word, check_als).  Checked before the
    device is; nothing else synchronises."""
    who = "als_solve_rows"
    R, nnz = _csr(who, rowptr, col, val, ("rowptr", "col", "val"))
    _vec1d(who, rows, "rows", torch.int64)
    B = rows.numel()
    if not torch.is_tensor(G) or G.dtype != torch.float32 or G.dim() != 2 or G.shape[0] != G.shape[1] or not G.is_contiguous():
        raise ValueError(f"{who}: G must be a contiguous (F, F) float32 tensor")
    F = _als_factors(who, T, G.shape[0])
    alpha = _finite(who, alpha, "alpha", 0.0)
    reg = _finite(who, reg, "reg", 0.0)
    if not reg > 0:
        raise ValueError(f"{who}: reg = {reg} is not > 0")
    if not isinstance(out_by_row, bool):
        raise ValueError(f"{who}: out_by_row = {out_by_row!r} is not a bool")
    block_bytes = _int_in(who, block_bytes, "block_bytes", 1, 2 ** 62)
    if out is None and out_by_row:
        raise ValueError(f"{who}: out_by_row writes into the caller's table: out is required")
    _out1d(who, flag, "flag", torch.int32, 1)
    out = _out2d(who, out, R if out_by_row else B, F, rowptr,
                 ((rowptr, "rowptr"), (col, "col"), (val, "val"), (rows, "rows"), (T, "T"), (G, "G"), (flag, "flag")), wider=True)
    lib = load_library()
    dev = rowptr.device
    if flag is None:
        flag = als_flag(dev)
    if plan is None:
        plan = als_plan(rowptr, rows, F, block_bytes)
    ldo = max(out.stride(0), F)
    for k0, k1, seg_base, seg_row, n_slots in plan:
        if not 0 <= k0 <= k1 <= B:
            raise ValueError(f"{who}: the plan lists rows [{k0}, {k1}) of {B}")
        scratch = torch.empty(n_slots * F * F, dtype=torch.float32, device=dev) if n_slots else None
        dst = out if out_by_row else out[k0:k1]
        _check(lib.ncf_als_solve_rows(_ptr(rowptr), _ptr(col), _ptr(val), nnz, R, _ptr(rows[k0:k1]), k1 - k0, _ptr(T), T.shape[0],
                                      max(T.stride(0), F), F, _ptr(G), alpha, reg, _ptr(dst), ldo, 1 if out_by_row else 0, _ptr(seg_base),
                                      _ptr(seg_row), n_slots, _ptr(scratch), _ptr(flag), _stream(rowptr)))
    return out


MMR_MAX_N, MMR_MAX_D, MMR_MAX_K = 256, 256, 128       # csrc/mmr.hip


def mmr_supported(N: int, D: int, K: int) -> bool:
    """Whether ncf_mmr_rerank takes a pool of ``N`` slots, vectors of ``D`` columns and ``K`` picks (host only)."""
    return bool(load_library().ncf_mmr_supported(int(N), int(D), int(K)))


def mmr_rerank(vectors: torch.Tensor, scores: torch.Tensor, positions: torch.Tensor, counts: Optional[torch.Tensor], k: int,
               lam: float = 0.5, normalize: bool = True):
    """Greedy MMR re-ranking of one candidate pool per user (ncf_mmr_rerank, THE CONTRACT in include/ncf_abi.h).  ``vectors``
    (n_items, D) fp32 rows (a column slice is fine), ``scores`` (B, N) fp32 and ``positions`` (B, N) int64 contiguous pools, ``counts``
    (B,) int32 slots in use per pool or None for N.  Returns ``(slot (B, k) int32, value (B, k) fp32, count (B,) int32)``: the pool
    slot picked at each step and its value when picked, -1 / -inf past ``count``.  A position >= n_items or < -1 is never picked and
    sets the sticky out-of-range flag (check_oob).  Shapes, dtypes and the kernel's limits are checked before the device is; one
    launch on the current stream, nothing synchronises."""
    who = "mmr_rerank"
    _table_f32(who, vectors, "vectors")
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.dim() != 2 or not scores.is_contiguous():
        raise ValueError(f"{who}: scores must be a contiguous (B, N) float32 tensor")
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 2 or not positions.is_contiguous():
        raise ValueError(f"{who}: positions must be a contiguous (B, N) int64 tensor")
    if positions.shape != scores.shape:
        raise ValueError(f"{who}: scores is {tuple(scores.shape)}, positions {tuple(positions.shape)}")
    B, N = scores.shape
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or not counts.is_contiguous()
                               or counts.numel() != B):
        raise ValueError(f"{who}: counts must be a contiguous ({B},) int32 tensor")
    n_items, D = vectors.shape
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"{who}: k = {k!r} is not an int")
    if not (1 <= N <= MMR_MAX_N and 4 <= D <= MMR_MAX_D and D % 4 == 0 and 1 <= k <= min(N, MMR_MAX_K)):
        raise ValueError(f"{who}: pool width N = {N}, vector width D = {D}, k = {k} is outside 1 <= N <= {MMR_MAX_N}, 4 <= D <= {MMR_MAX_D} "
                         f"with D % 4 == 0, 1 <= k <= min(N, {MMR_MAX_K})")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{who}: lam = {lam} is outside [0, 1]")
    _dev_all((vectors, "vectors"), (scores, "scores"), (positions, "positions"), (counts, "counts"))
    lib = load_library()
    dev = scores.device
    slot = torch.empty((B, k), dtype=torch.int32, device=dev)
    value = torch.empty((B, k), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    _check(lib.ncf_mmr_rerank(_ptr(vectors), n_items, D, vectors.stride(0), _ptr(scores), _ptr(positions), _ptr(counts), B, N, k, lam,
                              1 if normalize else 0, _ptr(slot), _ptr(value), _ptr(count), _ptr(_oob_flag(dev)), _stream(scores)))
    return slot, value, count


def folded_supported(N1: int, N2: int) -> bool:
    return bool(load_library().ncf_score_folded_supported(NCF_F32, int(N1), int(N2)))


def score_folded(PA: torch.Tensor, idxA, PB: torch.Tensor, idxB, packed_tail: PackedMLP, out: Optional[torch.Tensor] = None,
                 B: Optional[int] = None) -> torch.Tensor:
    """Folded-first-layer scoring: relu(PA[idxA] + PB[idxB]) -> tail MLP [N1 -> N2 -> 1] (packed_tail)."""
    lib = load_library()
    _dev(PA, "PA"), _dev(PB, "PB")
    rowsA, N1, ldA = _rows2d(PA, "PA")
    rowsB, N1b, ldB = _rows2d(PB, "PB")
    if N1 != N1b or packed_tail.dims[0] != N1 or packed_tail.n_layers != 2:
        raise ValueError("folded tables and tail MLP disagree")
    idxA, idxB = _idx(idxA), _idx(idxB)
    if B is None:
        B = idxA.numel() if idxA is not None else (idxB.numel() if idxB is not None else rowsA)
    if out is None:
        out = torch.empty((B, 1), dtype=torch.float32, device=PA.device)
    _check(lib.ncf_score_folded(NCF_F32, _ptr(PA), rowsA, ldA, _ptr(PB), rowsB, ldB, _ptr(idxA), _ptr(idxB), B, N1,
                                packed_tail.dims[1], _ptr(packed_tail.blob), _ptr(out), _ptr(_oob_flag(PA.device)), _stream(PA)))
    return out


def edge_softmax_csr(rowptr: torch.Tensor, col: torch.Tensor, attr: Optional[torch.Tensor], s: torch.Tensor,
                     out: Optional[torch.Tensor] = None, segments=None) -> torch.Tensor:
    """Per-destination softmax of the source scores times the edge weight (LightGAT).  ``segments`` = (segptr, row_of, seg_first) of
    the SpMM's split rows: the segmented form (parallel over segments: hub rows do not serialise on one wave)."""
    lib = load_library()
    _dev(s, "s")
    if out is None:
        out = torch.empty(max(col.numel(), 1), dtype=torch.float32, device=s.device)[:col.numel()]
    n_rows = rowptr.numel() - 1
    if segments is not None and segments[1] is not None:
        segptr, row_of, seg_first = segments
        n_seg = _gat_segments("edge_softmax_csr", segptr, row_of, seg_first, n_rows, col, ((attr, "attr"),))
        nbytes = lib.ncf_edge_softmax_segmented_workspace_bytes(n_seg, n_rows)
        _check(lib.ncf_edge_softmax_segmented(_ptr(segptr), _ptr(row_of), n_seg, _ptr(seg_first), n_rows, _ptr(col), _ptr(attr), _ptr(s), s.numel(),
                                              _ptr(out), _ptr(_gat_ws(None, nbytes, s.device)), nbytes, _stream(s)))
        return out
    _gat_segments("edge_softmax_csr", rowptr, None, None, n_rows, col, ((attr, "attr"),))
    _check(lib.ncf_edge_softmax_csr(_ptr(rowptr), _ptr(col), _ptr(attr), _ptr(s), n_rows, s.numel(), _ptr(out), _stream(s)))
    return out


def _gat_segments(fn, segptr, row_of, seg_first, n_rows, col, per_entry):
    """The refusals the edge softmax and the LightGAT wrappers share: level-0 segments of a CSR by destination (row_of None: its rows)
    and its per-entry arrays.  Returns the number of segments."""
    if segptr.dtype != torch.int64 or col.dtype != torch.int32 or not segptr.is_contiguous() or not col.is_contiguous():
        raise TypeError(f"{fn}: segptr must be contiguous int64 and col contiguous int32")
    n_seg = segptr.numel() - 1
    if row_of is not None:
        if row_of.dtype != torch.int32 or row_of.numel() != n_seg or not row_of.is_contiguous():
            raise TypeError(f"{fn}: row_of must be contiguous int32, one row per segment")
        if seg_first is None or seg_first.dtype != torch.int64 or seg_first.numel() != n_rows + 1 or not seg_first.is_contiguous():
            raise TypeError(f"{fn}: split rows need seg_first, contiguous int64 with n_rows + 1 entries")
    elif n_seg != n_rows:
        raise ValueError(f"{fn}: without row_of the segments are the rows")
    E = col.numel()
    for t, what in per_entry:
        if t is not None and (t.dtype != torch.float32 or t.numel() != E or not t.is_contiguous()):
            raise TypeError(f"{fn}: {what} must be contiguous float32, one element per CSR entry")
    return n_seg


def _gat_ws(workspace, nbytes, device):
    """The caller's workspace when it is large enough (contiguous uint8 on ``device``), else a fresh one."""
    if workspace is not None and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == device \
            and workspace.numel() >= max(nbytes, 4):
        return workspace
    return _workspace(nbytes, device)


def gat_edge_softmax(segptr: torch.Tensor, row_of: Optional[torch.Tensor], seg_first: Optional[torch.Tensor], n_rows: int, col: torch.Tensor,
                     attr: Optional[torch.Tensor], keep: Optional[torch.Tensor], s: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    """LightGAT's per-destination softmax over the KEPT entries (ncf_gat_edge_softmax): returns (alpha (E,), coef (E,) = attr * alpha;
    the same tensor when ``attr`` is None).  ``segptr`` / ``row_of`` / ``seg_first``: the level-0 segments of the prepared CSR
    (PreparedGraph.softmax_segments(); row_of None: segments are rows).  ``keep``: (E,) float32, 1 = kept, 0 = removed (the w of
    edge_keep called with attr = None); None: every entry kept, and coef is edge_softmax_csr's bit for bit.  ``workspace``: a
    contiguous uint8 buffer kept by the caller (PreparedGraph.gat_workspace(): one per graph); None or too small: one is allocated."""
    lib = load_library()
    _dev(s, "s")
    n_seg = _gat_segments("gat_edge_softmax", segptr, row_of, seg_first, n_rows, col, ((attr, "attr"), (keep, "keep")))
    if s.dtype != torch.float32 or not s.is_contiguous():
        raise TypeError("gat_edge_softmax: s must be contiguous float32")
    E = col.numel()
    alpha = torch.empty(E, dtype=torch.float32, device=s.device)
    coef = alpha if attr is None else torch.empty(E, dtype=torch.float32, device=s.device)
    if E == 0:                                # an edgeless graph: empty tensors carry null pointers
        return alpha, coef
    nbytes = lib.ncf_gat_edge_softmax_workspace_bytes(n_seg, n_rows) if row_of is not None else 0
    ws = _gat_ws(workspace, nbytes, s.device)
    _check(lib.ncf_gat_edge_softmax(_ptr(segptr), _ptr(row_of), n_seg, _ptr(seg_first), n_rows, _ptr(col), _ptr(attr), _ptr(keep), _ptr(s),
                                    s.numel(), _ptr(alpha), _ptr(coef) if attr is not None else None, _ptr(ws), nbytes, _stream(s)))
    return alpha, coef


def gat_edge_grad(segptr: torch.Tensor, row_of: Optional[torch.Tensor], seg_first: Optional[torch.Tensor], n_rows: int, col: torch.Tensor,
                  attr: Optional[torch.Tensor], alpha: torch.Tensor, dY: torch.Tensor, z: torch.Tensor, p: float = 0.0, seed: int = 0,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlogit (E,) of LightGAT's edge softmax (ncf_gat_edge_grad): alpha_e (g_e - S_r) with g_e = attr_e <dY[row_e], drop_e(z[col_e])>,
    the forward's message dropout (p, seed) regenerated per (CSR position, feature)."""
    lib = load_library()
    _dev(z, "z")
    _dev(dY, "dY")
    if alpha is None:
        raise TypeError("gat_edge_grad: alpha is required")
    n_seg = _gat_segments("gat_edge_grad", segptr, row_of, seg_first, n_rows, col, ((attr, "attr"), (alpha, "alpha")))
    Nz, D, ldz = _rows2d(z, "z")
    Ny, Dy, ldy = _rows2d(dY, "dY")
    if Dy != D or Ny != n_rows or z.dtype != torch.float32 or dY.dtype != torch.float32:
        raise TypeError("gat_edge_grad: dY must be (n_rows, D) and z (Nz, D), both float32")
    E = col.numel()
    dlogit = torch.empty(E, dtype=torch.float32, device=z.device)
    if E == 0:
        return dlogit
    nbytes = lib.ncf_gat_edge_grad_workspace_bytes(n_seg, n_rows)
    ws = _gat_ws(workspace, nbytes, z.device)
    _check(lib.ncf_gat_edge_grad(_ptr(segptr), _ptr(row_of), n_seg, _ptr(seg_first), n_rows, _ptr(col), _ptr(attr), _ptr(alpha), _ptr(dY), ldy,
                                 _ptr(z), Nz, ldz, D, float(p), int(seed) & 0xFFFFFFFF, _ptr(dlogit), _ptr(ws), nbytes, _stream(z)))
    return dlogit


def gat_source_reduce(csr_t: "SegmentedCSR", eid: torch.Tensor, dlogit: torch.Tensor) -> torch.Tensor:
    """ds (n_rows,) = the sum of dlogit[eid[k]] over each row of the CSR by source ``csr_t`` (PreparedGraph.transposed()), level by
    level over csr_t's segment tree like SegmentedCSR.spmm: ncf_gat_source_reduce on the entries, then on the partial sums of split
    rows.  The partial buffers are cached on ``csr_t``.  Empty rows give 0."""
    lib = load_library()
    _dev(dlogit, "dlogit")
    E = eid.numel()
    if eid.dtype != torch.int32 or not eid.is_contiguous() or E != csr_t.col.numel():
        raise TypeError("gat_source_reduce: eid must be contiguous int32, one id per entry of the transposed CSR")
    if dlogit.dtype != torch.float32 or not dlogit.is_contiguous() or dlogit.numel() != E:
        raise TypeError("gat_source_reduce: dlogit must be contiguous float32, one element per CSR entry")
    n = csr_t.n_rows
    out = torch.empty(n, dtype=torch.float32, device=dlogit.device)
    if E == 0:
        return out.zero_()
    levels = csr_t.levels
    bufs = csr_t._partials.get("gat_reduce")
    if bufs is None:
        bufs = [torch.empty(lv[0].numel() - 1, dtype=torch.float32, device=dlogit.device) for lv in levels[:-1]]
        csr_t._partials["gat_reduce"] = bufs
    idx, val = eid, dlogit
    for li, (segptr, row_of, edge_ids) in enumerate(levels):
        if li > 0:
            idx, val = edge_ids, bufs[li - 1]
        last = li == len(levels) - 1
        _check(lib.ncf_gat_source_reduce(_ptr(segptr), _ptr(row_of), segptr.numel() - 1, _ptr(idx), _ptr(val), val.numel(), _ptr(out), n,
                                         None if last else _ptr(bufs[li]), _stream(dlogit)))
    return out


def linear_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    """One layer with a selectable fused ReLU (the autograd wrappers keep every layer's output)."""
    lib = load_library()
    _dev(x, "x")
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise TypeError("linear_act needs fp32 activations and a contiguous fp32 weight")
    M, K, ldx = _rows2d(x, "x")
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError("weight / activation widths disagree")
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _check(lib.ncf_linear_forward(NCF_F32, _ptr(x), M, ldx, _ptr(weight), _ptr(bias), K, N, 1 if relu else 0, _ptr(out), N, _stream(x)))
    return out


LINEAR_FORMS = {0: "none", 1: "tiled", 2: "rowdot", 3: "rs", 4: "rsp"}    # ncf_linear_plan's *form


def linear_plan(M: int, N: int, K: int):
    """(form, nt, kslices, col_blocks, grid_x) of the kernel a Linear of M rows, N outputs and K inputs runs under the current
    linear_kernel / linear_kslices options; form by name (LINEAR_FORMS).  Host only: no launch, no device."""
    form, *rest = _query(load_library().ncf_linear_plan, (int(M), int(N), int(K)), (_c_int, _c_int, _c_int, _c_int, _c_i64))
    return (LINEAR_FORMS[form], *rest)


# ------------------------------------------------------------------ backward (training step)
def gemm_tn(A: torch.Tensor, Bm: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (N1, N2) = A^T @ Bm for A (M, N1), Bm (M, N2): the weight gradient dW = dY^T X."""
    lib = load_library()
    _dev(A, "A"), _dev(Bm, "B")
    M, N1, lda = _rows2d(A, "A")
    M2, N2, ldb = _rows2d(Bm, "B")
    if M != M2 or A.dtype != torch.float32 or Bm.dtype != torch.float32:
        raise ValueError("gemm_tn needs fp32 operands with the same number of rows")
    if out is None:
        out = torch.empty((N1, N2), dtype=torch.float32, device=A.device)
    nb = lib.ncf_gemm_tn_workspace_bytes(M, N1, N2)
    ws = _workspace(nb, A.device)
    _check(lib.ncf_gemm_tn(_ptr(A), lda, _ptr(Bm), ldb, M, N1, N2, _ptr(out), out.stride(0), _ptr(ws), nb, _stream(A)))
    return out


def colsum(X: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    _dev(X, "X")
    M, N, ld = _rows2d(X, "X")
    out = torch.empty(N, dtype=torch.float32, device=X.device)
    nb = lib.ncf_colsum_workspace_bytes(M, N)
    ws = _workspace(nb, X.device)
    _check(lib.ncf_colsum(_ptr(X), ld, M, N, _ptr(out), _ptr(ws), nb, _stream(X)))
    return out


def relu_backward_(dY: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    M, N, ldd = _rows2d(dY, "dY")
    _, _, ldy = _rows2d(Y, "Y")
    _check(lib.ncf_relu_backward(_ptr(dY), ldd, _ptr(Y), ldy, M, N, _stream(dY)))
    return dY


def relu_backward(dY: torch.Tensor, Y: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """scale * dY masked by Y > 0 into a NEW tensor (dY untouched)."""
    lib = load_library()
    _dev(dY, "dY"), _dev(Y, "Y")
    M, N, ldd = _rows2d(dY, "dY")
    M2, N2, ldy = _rows2d(Y, "Y")
    if (M, N) != (M2, N2):
        raise ValueError("dY and Y shapes disagree")
    out = torch.empty((M, N), dtype=torch.float32, device=dY.device)
    _check(lib.ncf_relu_backward_out(_ptr(dY), ldd, _ptr(Y), ldy, _ptr(out), N, M, N, float(scale), _stream(dY)))
    return out


def scatter_add_rows(src: torch.Tensor, idx: Optional[torch.Tensor], dst: torch.Tensor) -> torch.Tensor:
    """dst[idx[p], :] += src[p, :] (src may be a column slice of a wider matrix)."""
    lib = load_library()
    _dev(src, "src"), _dev(dst, "dst")
    B, E, lds = _rows2d(src, "src")
    rows, E2, ldd = _rows2d(dst, "dst")
    if E != E2:
        raise ValueError("row widths disagree")
    _check(lib.ncf_scatter_add_rows(_ptr(src), lds, _ptr(_idx(idx)), B, E, _ptr(dst), ldd, rows, _ptr(_oob_flag(src.device)), _stream(src)))
    return dst


# ------------------------------------------------------------------ training step: Linear-layout embeddings, Adam
def gather_cols(W: torch.Tensor, bias: Optional[torch.Tensor], idx: torch.Tensor) -> torch.Tensor:
    """out[p, :] = W[:, idx[p]] + bias  (W is the nn.Linear weight [E, U])."""
    lib = load_library()
    _dev(W, "W")
    E, U, ldw = _rows2d(W, "W")
    idx = _idx(idx)
    out = torch.empty((idx.numel(), E), dtype=torch.float32, device=W.device)
    _check(lib.ncf_gather_cols(_ptr(W), ldw, _ptr(bias), _ptr(idx), idx.numel(), E, U, _ptr(out), out.stride(0) if idx.numel() else E,
                               _ptr(_oob_flag(W.device)), _stream(W)))
    return out


def scatter_add_cols(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[:, idx[p]] += src[p, :]  (dst is [E, U])."""
    lib = load_library()
    _dev(src, "src")
    B, E, lds = _rows2d(src, "src")
    E2, U, ldd = _rows2d(dst, "dst")
    if E != E2:
        raise ValueError("scatter_add_cols: widths disagree")
    _check(lib.ncf_scatter_add_cols(_ptr(src), lds, _ptr(_idx(idx)), B, E, _ptr(dst), ldd, U, _ptr(_oob_flag(src.device)), _stream(src)))
    return dst


def adam_step_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int):
    lib = load_library()
    _dev(p, "p")
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError("adam_step_: contiguous fp32 tensors of one size")
    _check(lib.ncf_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                             float(weight_decay), int(step), _stream(p)))


def adam_rows_(p: torch.Tensor, m: torch.Tensor, v: torch.Tensor, ids: torch.Tensor, g: torch.Tensor, lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int):
    """Row-sparse Adam, in place: rows ``ids`` of the id-major ``[rows, E]`` buffers ``p`` / ``m`` / ``v`` (one row stride) take ONE
    Adam update each, with the sum of their gradient rows ``g[o]`` (``ids[o]`` = the row occurrence ``o`` belongs to; ``g`` may be
    a column slice of a wider matrix).  Untouched rows are not read or written: weight decay and the moments' decay reach
    touched rows only.  The ids are ordered by a stable ``torch.sort`` on the current stream; nothing synchronises with the
    host.  Deterministic (no atomics); an id outside ``[0, rows)`` is skipped and raises at the next ``check_oob``."""
    lib = load_library()
    _dev(p, "p"), _dev(g, "g"), _dev(ids, "ids")
    rows, E, ld = _rows2d(p, "p")
    for t, what in ((m, "m"), (v, "v")):
        _dev(t, what)
        if t.dtype != torch.float32 or t.shape != p.shape or t.stride() != p.stride():
            raise ValueError(f"adam_rows_: {what} must be fp32 with p's shape and strides")
    n, Eg, ldg = _rows2d(g, "g")
    ids = _idx(ids)
    if p.dtype != torch.float32 or g.dtype != torch.float32 or Eg != E or ids.numel() != n:
        raise ValueError("adam_rows_: fp32 p and g of one row width, one id per gradient row")
    if not (p.device == m.device == v.device == g.device == ids.device):
        raise ValueError("adam_rows_: tensors on different devices")
    if n == 0:
        return
    order, perm = torch.sort(ids, stable=True)
    _check(lib.ncf_adam_rows(_ptr(p), _ptr(m), _ptr(v), ld, rows, E, _ptr(order), _ptr(perm), n, _ptr(g), ldg, float(lr), float(beta1),
                             float(beta2), float(eps), float(weight_decay), int(step), _ptr(_oob_flag(p.device)), _stream(p)))


# ------------------------------------------------------------------ negative sampling (pair-wise training)
def _csr_rowptr(rowptr: torch.Tensor, what: str) -> int:
    _dev(rowptr, what)
    if rowptr.dtype != torch.int64 or rowptr.dim() != 1 or not rowptr.is_contiguous() or rowptr.numel() < 1:
        raise ValueError(f"{what} must be a contiguous 1-D int64 tensor of rows + 1 entries")
    return rowptr.numel() - 1


def negative_cdf(rowptr: torch.Tensor, rating: torch.Tensor, w: float, out: Optional[torch.Tensor] = None,
                 flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ncf_negative_cdf: every row's normalised inclusive prefix of its weights (1 when w == 0, rating ** w otherwise), each row
    ending in exactly 1.0 — np.random.choice's CDF for _negative_sampling_probs (datasets/base.py:57-70).  ``flag`` (int32, 1
    element; default: the device's out-of-range flag) is set when a row's total is not finite and positive.  No synchronisation."""
    lib = load_library()
    rows = _csr_rowptr(rowptr, "rowptr")
    _dev(rating, "rating")
    if rating.dtype != torch.float32 or rating.dim() != 1 or not rating.is_contiguous():
        raise ValueError("rating must be a contiguous 1-D fp32 tensor")
    if out is None:
        out = torch.empty_like(rating)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rating.numel():
        raise ValueError("out must be a contiguous fp32 tensor of the ratings' length")
    flag = _oob_flag(rating.device) if flag is None else flag
    _check(lib.ncf_negative_cdf(_ptr(rowptr), rows, _ptr(rating), float(w), _ptr(out), _ptr(flag), _stream(rating)))
    return out


def sample_negatives(rowptr: torch.Tensor, cdf: torch.Tensor, neg: torch.Tensor, pick: torch.Tensor, seed: int, slot0: int = 0,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ncf_sample_negatives: out[b] = neg[rowptr[r] + j] (int64) for r = pick[b], j = searchsorted(cdf row r, u_b, 'right') with u_b
    the header's hash of (seed, slot0 + b).  A pick outside the rows writes -1 and sets the out-of-range flag (IndexError at the
    next check_oob).  No synchronisation."""
    lib = load_library()
    rows = _csr_rowptr(rowptr, "rowptr")
    _dev(cdf, "cdf"), _dev(neg, "neg")
    if cdf.dtype != torch.float32 or not cdf.is_contiguous() or neg.dtype != torch.int32 or not neg.is_contiguous() or cdf.numel() != neg.numel():
        raise ValueError("cdf (fp32) and neg (int32) must be contiguous and of one length")
    pick = _idx(pick)
    n = pick.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=cdf.device)
    if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != n:
        raise ValueError("out must be a contiguous int64 tensor of n entries")
    _check(lib.ncf_sample_negatives(_ptr(rowptr), _ptr(cdf), _ptr(neg), rows, _ptr(pick), n, int(seed) & 0xFFFFFFFF, int(slot0), _ptr(out),
                                    _ptr(_oob_flag(cdf.device)), _stream(cdf)))
    return out


UNSEEN_MAX_K, UNSEEN_LANE_K = 1024, 8       # include/ncf_abi.h NCF_UNSEEN_*


def unseen_flag(device) -> torch.Tensor:
    """The sticky int32 flag word of ncf_sample_unseen on ``device`` (UNSEEN_FLAG_*)."""
    return _flag("unseen", device)


def check_unseen(device, flag: Optional[torch.Tensor] = None):
    """Synchronising check of sample_unseen's flag word: raises, and clears it, when a call met a pick outside the users (IndexError)
    or a user with fewer unseen items than the draws asked for (ValueError); such rows were written as -1."""
    _check_flag("unseen", device, flag)


def sample_unseen(seen: tuple, n_items: int, pick: torch.Tensor, k: int, seed: int, slot0: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ncf_sample_unseen: ``(n, k)`` int64 — row b holds k distinct items of [0, n_items) that user pick[b] has not seen, each uniform
    over what is left, a fixed function of (seed, slot0 + b) and the user's row of ``seen`` = (rowptr (users + 1) int64, col int32
    strictly ascending inside a row): THE CONTRACT in include/ncf_abi.h.  No rejection rounds, no host read.  k <= UNSEEN_LANE_K runs one
    lane per row, a larger k one wave per row.  A pick outside the users or a user with fewer than k unseen items gets a row of -1
    and raises at the next check_unseen.  No synchronisation."""
    who = "sample_unseen"
    if not (isinstance(seen, (tuple, list)) and len(seen) == 2 and all(torch.is_tensor(t) and t.dim() == 1 for t in seen)):
        raise ValueError(f"{who}: seen = (rowptr int64 (users + 1), col int32)")
    rowptr, col = seen
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or not rowptr.is_contiguous() or not col.is_contiguous() or rowptr.numel() < 1:
        raise ValueError(f"{who}: seen = (rowptr int64 (users + 1), col int32), both contiguous")
    n_items = _int_in(who, n_items, "n_items", 1, 2 ** 31 - 1)
    k = _int_in(who, k, "k", 1, UNSEEN_MAX_K)
    slot0 = _int_in(who, slot0, "slot0", 0, 2 ** 62)
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
        raise ValueError(f"{who}: seed = {seed!r} is not an integer")
    if not torch.is_tensor(pick) or pick.dtype != torch.int64 or pick.dim() != 1 or not pick.is_contiguous():
        raise ValueError(f"{who}: pick must be a contiguous 1-D int64 tensor")
    n = pick.numel()
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (n, k)):
        raise ValueError(f"{who}: out must be a contiguous ({n}, {k}) int64 tensor")
    _dev_all((rowptr, "seen rowptr"), (col, "seen col"), (pick, "pick"), (out, "out"))
    lib = load_library()
    if out is None:
        out = torch.empty((n, k), dtype=torch.int64, device=pick.device)
    _check(lib.ncf_sample_unseen(_ptr(rowptr), _ptr(col), rowptr.numel() - 1, n_items, _ptr(pick), n, k, int(seed) & 0xFFFFFFFF, slot0,
                                 _ptr(out), _ptr(_flag("unseen", pick.device)), _stream(pick)))
    return out


# ------------------------------------------------------------------ top-K
TOPK_MAX_K = 1024


def topk_rows(scores: torch.Tensor, k: int, seen: Optional[tuple] = None):
    """(out_score (R, k) fp32, out_idx (R, k) int32, out_count (R,) int32) of ncf_topk_rows: each row's k best columns in the order
    of torch.sort(descending=True, stable=True) (NaN last), skipping the columns listed for the row in ``seen`` = (rowptr (R + 1)
    int64, col int32), a CSR on the GPU.  Slots past out_count hold idx -1 / score -inf.  Outputs and workspace come from the
    caching allocator on the current stream; no host synchronisation."""
    lib = load_library()
    _dev(scores, "scores")
    if scores.dtype != torch.float32:
        raise TypeError("topk_rows takes fp32 scores")
    R, C, ld = _rows2d(scores, "scores")
    k = int(k)
    rowptr, col = _csr_pair(seen, R, scores.device, "seen")
    nbytes = lib.ncf_topk_workspace_bytes(R, C, k)
    out_score, out_idx, out_count, ws = _topk_outputs(R, k, nbytes, scores.device)
    _check(lib.ncf_topk_rows(_ptr(scores), R, C, ld, _ptr(rowptr), _ptr(col), k, _ptr(out_score), _ptr(out_idx), _ptr(out_count),
                             _ptr(ws), nbytes, _stream(scores)))
    return out_score, out_idx, out_count


DOT_TOPK_MAX_K = 128     # the fused kernel's limits (include/ncf_abi.h ncf_dot_topk); outside them it returns NCF_EUNSUPPORTED
DOT_TOPK_MAX_D = 256


def _topk_outputs(R, k, nbytes, dev):
    """(out_score (R, k) fp32, out_idx (R, k) int32, out_count (R,) int32, workspace of at least nbytes) of a top-K call, from the
    caching allocator."""
    out_score = torch.empty((R, max(k, 0)), dtype=torch.float32, device=dev)
    out_idx = torch.empty((R, max(k, 0)), dtype=torch.int32, device=dev)
    out_count = torch.empty(R, dtype=torch.int32, device=dev)
    ws = _workspace(nbytes, dev)
    return out_score, out_idx, out_count, ws


def _csr_pair(pair, R, dev, what, required=False):
    """The CSR ``pair`` = (rowptr (R + 1) int64, col int32) of a ranking call as the kernels take it; ``what``: "seen" (None allowed:
    nothing to skip) or "targets" (required)."""
    if pair is None:
        if required:
            raise ValueError(f"{what} = (rowptr int64 (R + 1), col int32) is required")
        return None, None
    rowptr, col = pair
    if not (rowptr.is_cuda and col.is_cuda):          # the messages are formatted only when one is raised
        _dev(rowptr, f"{what} rowptr"), _dev(col, f"{what} col")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or rowptr.dim() != 1 or col.dim() != 1:
        raise ValueError(f"{what} = (rowptr int64 (R + 1), col int32)")
    if rowptr.numel() != R + 1:
        raise ValueError(f"{what} rowptr has {rowptr.numel()} entries, {R + 1} expected")
    rowptr, col = rowptr.contiguous(), col.contiguous()
    if col.numel() == 0 and not required:     # a valid exclusion CSR with no entries: nothing to skip (targets: _rank_outputs)
        col = torch.empty(1, dtype=torch.int32, device=dev)
    return rowptr, col


def _dot_operands(fn, tabA, idxA, tabB, idxB):
    """The operands dot_topk and dot_rank share, checked for the public function ``fn``: (the ABI arguments up to D, (B, I, D, dev))."""
    _dev(tabA, "tabA"), _dev(tabB, "tabB")
    if tabA.dtype != torch.float32 or tabB.dtype != torch.float32:
        raise TypeError(f"{fn} takes fp32 tables")
    rowsA, D, ldA = _rows2d(tabA, "tabA")
    rowsB, DB, ldB = _rows2d(tabB, "tabB")
    if D != DB:
        raise ValueError(f"{fn} needs equal widths")
    idxA, idxB = _idx(idxA), _idx(idxB)
    B = idxA.numel() if idxA is not None else rowsA
    I = idxB.numel() if idxB is not None else rowsB
    return (_ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(idxA), _ptr(idxB), B, I, D), (B, I, D, tabA.device)


def _gmf_operands(fn, tabA, tabB, gmf):
    """The GMF term ``gmf`` = (gmfA, gmfB, w) of a NeuMF call, checked for the public function ``fn`` against the tower's tables:
    (D, ldGA, ldGB)."""
    gmfA, gmfB, w = gmf
    _table_f32(fn, gmfA, "gmfA"), _table_f32(fn, gmfB, "gmfB")
    D = gmfA.shape[1]
    if gmfB.shape[1] != D:
        raise ValueError(f"{fn}: the GMF tables are {D} and {gmfB.shape[1]} wide")
    if gmfA.shape[0] != tabA.shape[0] or gmfB.shape[0] != tabB.shape[0]:
        raise ValueError(f"{fn}: a GMF table must have the rows of its side's tower table "
                         f"({gmfA.shape[0]} / {tabA.shape[0]} users, {gmfB.shape[0]} / {tabB.shape[0]} items)")
    _vec1d(fn, w, "w", torch.float32, D)
    _dev_all((gmfA, "gmfA"), (gmfB, "gmfB"), (w, "w"))
    return D, gmfA.stride(0), gmfB.stride(0)


def _mlp_operands(fn, tabA, idxA, tabB, idxB, packed, user_first, gmf=None):
    """The operands mlp_topk and mlp_rank share, checked for the public function ``fn``: (the ABI arguments up to the packed blob,
    (B, I, dims array, dev)).  user_first=False: the users are tabB's rows and idxB.  With ``gmf`` = (gmfA, gmfB, w) the arguments
    are those of the NeuMF entries (users first), up to w."""
    _dev(tabA, "tabA"), _dev(tabB, "tabB")
    rowsA, EA, ldA = _rows2d(tabA, "tabA")
    rowsB, EB, ldB = _rows2d(tabB, "tabB")
    if tabA.dtype != tabB.dtype:
        raise TypeError(f"{fn}: both tables must have one dtype")
    if tabA.dtype != packed.dtype:
        raise TypeError(f"tables are {tabA.dtype} but the MLP was packed for {packed.dtype}")
    idxA, idxB = _idx(idxA), _idx(idxB)
    nA = idxA.numel() if idxA is not None else rowsA
    nB = idxB.numel() if idxB is not None else rowsB
    user_ids, item_ids, B, I = (idxA, idxB, nA, nB) if user_first else (idxB, idxA, nB, nA)
    d = _dims_array(packed.dims)
    if gmf is not None:
        if not user_first:
            raise ValueError(f"{fn}: users first only")
        D, ldGA, ldGB = _gmf_operands(fn, tabA, tabB, gmf)
        args = (packed.dt, _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, _ptr(gmf[0]), ldGA, _ptr(gmf[1]), ldGB, EA, EB, D, _ptr(user_ids),
                _ptr(item_ids), B, I, packed.n_layers, d, _ptr(packed.blob), _ptr(gmf[2]))
        return args, (B, I, d, tabA.device)
    args = (packed.dt, _ptr(tabA), rowsA, ldA, _ptr(tabB), rowsB, ldB, EA, EB, 1 if user_first else 0, _ptr(user_ids), _ptr(item_ids), B, I,
            packed.n_layers, d, _ptr(packed.blob))
    return args, (B, I, d, tabA.device)


def dot_topk(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], k: int,
             seen: Optional[tuple] = None):
    """ncf_dot_topk: for each user row tabA[idxA[r]] (tabA[r] with idxA None) the k best columns c of the list idxB (every row of
    tabB with idxB None) by <user row, tabB[idxB[c]]> — exactly ``topk_rows(gather_dot(...).view(B, I), k, seen)``, bit for bit,
    without the B x I score matrix.  Returns (out_score (B, k) fp32, out_idx (B, k) int32 columns of the list, out_count (B,)
    int32) like topk_rows.  fp32 tables only; k <= DOT_TOPK_MAX_K and width <= DOT_TOPK_MAX_D, else NativeError with code
    NCF_EUNSUPPORTED and nothing launched.  Outputs and workspace from the caching allocator on the current stream; no sync."""
    lib = load_library()
    args, (B, I, D, dev) = _dot_operands("dot_topk", tabA, idxA, tabB, idxB)
    k = int(k)
    rowptr, col = _csr_pair(seen, B, dev, "seen")
    nbytes = lib.ncf_dot_topk_workspace_bytes(B, I, D, k)
    out_score, out_idx, out_count, ws = _topk_outputs(B, k, nbytes, dev)
    _check(lib.ncf_dot_topk(*args, _ptr(rowptr), _ptr(col), k, _ptr(out_score), _ptr(out_idx), _ptr(out_count), _ptr(ws), nbytes,
                            _ptr(_oob_flag(dev)), _stream(tabA)))
    return out_score, out_idx, out_count


MLP_TOPK_MAX_K = 128     # the fused MLP kernel's limit on k (include/ncf_abi.h ncf_mlp_topk)


def mlp_topk_supported(packed: PackedMLP, EA: int, EB: int, k: int) -> bool:
    """Whether ncf_mlp_topk has a kernel for this packed MLP, split (EA, EB) and k."""
    return bool(load_library().ncf_mlp_topk_supported(packed.dt, EA, EB, packed.n_layers, _dims_array(packed.dims), int(k)))


def mlp_topk(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], packed: PackedMLP,
             k: int, seen: Optional[tuple] = None, user_first: bool = True):
    """ncf_mlp_topk: the k best items of each user for an MLP readout over cat(tabA[idxA[.]], tabB[idxB[.]]) (id lists None =
    every row).  user_first=True: the users are the first part (rows of the result = idxA, ranked columns = idxB); False: the items
    are (columns = idxA, rows = idxB).  Exactly ``topk_rows(score_fused(...).view(B, I), k, seen)`` over every (user, item) pair,
    bit for bit, without the pair id columns or the score matrix.  Returns (out_score (B, k) fp32, out_idx (B, k) int32 columns
    of the list, out_count (B,) int32) like topk_rows.  A shape without a fused instance, a bf16 blob or k > MLP_TOPK_MAX_K raise
    NativeError with code NCF_EUNSUPPORTED and launch nothing.  Outputs and workspace from the caching allocator on the current
    stream; no sync."""
    return _mlp_topk("mlp_topk", tabA, idxA, tabB, idxB, packed, k, seen, user_first, None)


def _mlp_topk(fn, tabA, idxA, tabB, idxB, packed, k, seen, user_first, gmf):
    """mlp_topk (``gmf`` None) and neumf_topk (``gmf`` = (gmfA, gmfB, w)): one marshalling, the entry and its workspace query differ."""
    lib = load_library()
    args, (B, I, d, dev) = _mlp_operands(fn, tabA, idxA, tabB, idxB, packed, user_first, gmf)
    k = int(k)
    rowptr, col = _csr_pair(seen, B, dev, "seen")
    if gmf is None:
        entry, nbytes = lib.ncf_mlp_topk, lib.ncf_mlp_topk_workspace_bytes(B, I, 1 if user_first else 0, packed.n_layers, d, k)
    else:
        entry, nbytes = lib.ncf_neumf_topk, lib.ncf_neumf_topk_workspace_bytes(B, I, packed.n_layers, d, gmf[0].shape[1], k)
    out_score, out_idx, out_count, ws = _topk_outputs(B, k, nbytes, dev)
    _check(entry(*args, _ptr(rowptr), _ptr(col), k, _ptr(out_score), _ptr(out_idx), _ptr(out_count), _ptr(ws), nbytes,
                 _ptr(_oob_flag(dev)), _stream(tabA)))
    return out_score, out_idx, out_count


# ------------------------------------------------------------------ exact ranks
RANK_MAX_TARGETS = 128   # targets per row of a fused rank call (include/ncf_abi.h ncf_rank_max_targets); rank_rows takes any number
DOT_RANK_MAX_D = 256     # the fused dot-product kernel's width limit, as DOT_TOPK_MAX_D


def _rank_overflow_flag(device) -> torch.Tensor:
    return _flag("rank_overflow", device)


def check_rank_overflow(device):
    """Synchronising check of the sticky flag a fused rank call sets when a row has more targets than its ``max_targets``."""
    _check_flag("rank_overflow", device)


def _rank_outputs(R, col, nbytes, dev, rank):
    """(rank (n_targets,) int32, ranked (R,) int32, workspace, col and rank as the kernel takes them) of a rank call, from the caching
    allocator.  A caller that ranks blocks of rows against one target CSR passes its own ``rank`` (every block writes its rows'
    entries)."""
    n = col.numel()
    if rank is None:
        rank = torch.empty(n, dtype=torch.int32, device=dev)
    elif rank.dtype != torch.int32 or rank.numel() != n or not rank.is_contiguous() or rank.device != dev:
        raise ValueError("rank must be a contiguous int32 tensor with one entry per target")
    ranked = torch.empty(R, dtype=torch.int32, device=dev)
    ws = _workspace(nbytes, dev)
    rank_arg = rank
    if n == 0:                                  # a valid CSR with no entries: the kernels still want pointers
        col = torch.empty(1, dtype=torch.int32, device=dev)
        rank_arg = torch.empty(1, dtype=torch.int32, device=dev)
    return rank, ranked, ws, col, rank_arg


def rank_rows(scores: torch.Tensor, targets: tuple, seen: Optional[tuple] = None, rank: Optional[torch.Tensor] = None):
    """ncf_rank_rows: ``(rank (n_targets,) int32, ranked (R,) int32)`` — for every entry of the target CSR ``targets`` = (rowptr
    (R + 1) int64, col int32) the number of columns of its row of ``scores`` (R, C) fp32 that are not in ``seen`` (a CSR like
    topk_rows') and come before the target in topk_rows' order, i.e. the slot the target would hold in an unbounded topk_rows
    result; -1 for a target that is excluded or outside [0, C).  ranked[r]: the number of non-excluded columns of row r.  Entry
    e = rowptr[r] + i of row r indexes col and rank, so a slice of a longer rowptr ranks a block of rows into a shared ``rank``.
    Any number of targets per row.  Outputs and workspace from the caching allocator on the current stream; no sync."""
    lib = load_library()
    _dev(scores, "scores")
    if scores.dtype != torch.float32:
        raise TypeError("rank_rows takes fp32 scores")
    R, C, ld = _rows2d(scores, "scores")
    dev = scores.device
    rowptr, col = _csr_pair(seen, R, dev, "seen")
    trow, tcol = _csr_pair(targets, R, dev, "targets", required=True)
    n = tcol.numel()
    nbytes = lib.ncf_rank_rows_workspace_bytes(R, C, n)
    rank, ranked, ws, tcol, rank_arg = _rank_outputs(R, tcol, nbytes, dev, rank)
    _check(lib.ncf_rank_rows(_ptr(scores), R, C, ld, _ptr(rowptr), _ptr(col), _ptr(trow), _ptr(tcol), n, _ptr(rank_arg), _ptr(ranked),
                             _ptr(ws), nbytes, _stream(scores)))
    return rank, ranked


def dot_rank(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], targets: tuple,
             max_targets: int, seen: Optional[tuple] = None, rank: Optional[torch.Tensor] = None):
    """ncf_dot_rank: exactly ``rank_rows(gather_dot(...).view(B, I), targets, seen)`` for the users tabA[idxA[.]] against the list
    idxB of rows of tabB (arguments as dot_topk), without the B x I score matrix.  ``max_targets`` (1 .. RANK_MAX_TARGETS) bounds the
    targets per row and sizes the kernel's LDS; 1 is the leave-one-out form.  A row with more targets has only its first
    max_targets ranked (the others -1) and sets the sticky flag check_rank_overflow() reads.  fp32 tables, width <= DOT_RANK_MAX_D,
    else NativeError (NCF_EUNSUPPORTED) and nothing launched.  No sync."""
    lib = load_library()
    args, (B, I, D, dev) = _dot_operands("dot_rank", tabA, idxA, tabB, idxB)
    rowptr, col = _csr_pair(seen, B, dev, "seen")
    trow, tcol = _csr_pair(targets, B, dev, "targets", required=True)
    n, max_targets = tcol.numel(), int(max_targets)
    nbytes = lib.ncf_dot_rank_workspace_bytes(B, I, D, n, max_targets)
    rank, ranked, ws, tcol, rank_arg = _rank_outputs(B, tcol, nbytes, dev, rank)
    _check(lib.ncf_dot_rank(*args, _ptr(rowptr), _ptr(col), _ptr(trow), _ptr(tcol), n, max_targets, _ptr(rank_arg), _ptr(ranked), _ptr(ws),
                            nbytes, _ptr(_oob_flag(dev)), _ptr(_rank_overflow_flag(dev)), _stream(tabA)))
    return rank, ranked


def mlp_rank_supported(packed: PackedMLP, EA: int, EB: int, max_targets: int = 1) -> bool:
    """Whether ncf_mlp_rank has a kernel for this packed MLP, split (EA, EB) and max_targets."""
    return bool(load_library().ncf_mlp_rank_supported(packed.dt, EA, EB, packed.n_layers, _dims_array(packed.dims), int(max_targets)))


def mlp_rank(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], packed: PackedMLP,
             targets: tuple, max_targets: int, seen: Optional[tuple] = None, user_first: bool = True,
             rank: Optional[torch.Tensor] = None):
    """ncf_mlp_rank: exactly ``rank_rows(score_fused(...).view(B, I), targets, seen)`` over every (user, item) pair of an MLP readout
    (arguments as mlp_topk), without the pair id columns or the score matrix.  max_targets and the overflow flag as dot_rank.  A
    shape without a fused instance or a bf16 blob raise NativeError (NCF_EUNSUPPORTED) and launch nothing.  No sync."""
    return _mlp_rank("mlp_rank", tabA, idxA, tabB, idxB, packed, targets, max_targets, seen, user_first, rank, None)


def _mlp_rank(fn, tabA, idxA, tabB, idxB, packed, targets, max_targets, seen, user_first, rank, gmf):
    """mlp_rank (``gmf`` None) and neumf_rank (``gmf`` = (gmfA, gmfB, w)), as _mlp_topk."""
    lib = load_library()
    args, (B, I, d, dev) = _mlp_operands(fn, tabA, idxA, tabB, idxB, packed, user_first, gmf)
    rowptr, col = _csr_pair(seen, B, dev, "seen")
    trow, tcol = _csr_pair(targets, B, dev, "targets", required=True)
    n, max_targets = tcol.numel(), int(max_targets)
    if gmf is None:
        entry, nbytes = lib.ncf_mlp_rank, lib.ncf_mlp_rank_workspace_bytes(B, I, 1 if user_first else 0, packed.n_layers, d, n, max_targets)
    else:
        entry, nbytes = lib.ncf_neumf_rank, lib.ncf_neumf_rank_workspace_bytes(B, I, packed.n_layers, d, gmf[0].shape[1], n, max_targets)
    rank, ranked, ws, tcol, rank_arg = _rank_outputs(B, tcol, nbytes, dev, rank)
    _check(entry(*args, _ptr(rowptr), _ptr(col), _ptr(trow), _ptr(tcol), n, max_targets, _ptr(rank_arg), _ptr(ranked), _ptr(ws),
                 nbytes, _ptr(_oob_flag(dev)), _ptr(_rank_overflow_flag(dev)), _stream(tabA)))
    return rank, ranked


# ------------------------------------------------------------------ NeuMF: the MLP tower plus a GMF term (include/ncf_abi.h ncf_neumf_score)
NEUMF_MAX_D = 128        # the GMF width: a multiple of 8 in 8 .. 128


def neumf_supported(packed: PackedMLP, EA: int, EB: int, D: int) -> bool:
    """Whether the NeuMF kernels take this packed tower (its last layer: predict.weight[:, D:] and predict.bias), split (EA, EB) and
    GMF width D."""
    return bool(load_library().ncf_neumf_supported(packed.dt, int(EA), int(EB), int(D), packed.n_layers, _dims_array(packed.dims)))


def neumf_score(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], gmfA: torch.Tensor,
                gmfB: torch.Tensor, packed: PackedMLP, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ncf_neumf_score: (B, 1) fp32 scores of the pairs (idxA[b], idxB[b]) (a list None: position b) — the tower over cat(tabA row,
    tabB row) with ``packed``, plus the GMF term over the rows of gmfA / gmfB weighted by ``w`` (D floats), in the header's operation
    order.  One launch, no sync.  A shape the kernel does not take raises NativeError (NCF_EUNSUPPORTED)."""
    lib = load_library()
    args, (B, I, d, dev) = _mlp_operands("neumf_score", tabA, idxA, tabB, idxB, packed, True, (gmfA, gmfB, w))
    if idxA is not None and idxB is not None and B != I:
        raise ValueError(f"neumf_score: {B} user ids and {I} item ids")
    n = B if idxA is not None else I if idxB is not None else min(B, I)
    if out is None:
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
    _out1d("neumf_score", out, "out", torch.float32, n)
    _dev(out, "out")
    (dt, pA, rowsA, ldA, pB, rowsB, ldB, pGA, ldGA, pGB, ldGB, EA, EB, D, pU, pI, _, _, n_layers, d, blob, pw) = args
    _check(lib.ncf_neumf_score(dt, pA, rowsA, ldA, pB, rowsB, ldB, pGA, ldGA, pGB, ldGB, pU, pI, n, EA, EB, D, n_layers, d, blob, pw,
                               _ptr(out), _ptr(_oob_flag(dev)), _stream(tabA)))
    return out


def neumf_topk(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], gmfA: torch.Tensor,
               gmfB: torch.Tensor, packed: PackedMLP, w: torch.Tensor, k: int, seen: Optional[tuple] = None):
    """ncf_neumf_topk: exactly ``topk_rows(neumf_score over every (user, item) pair, k, seen)``, bit for bit, without the score
    matrix; users first.  Arguments, results, limits and refusals as mlp_topk; ``ranking_plan("mlp_topk", ...)`` is its plan."""
    return _mlp_topk("neumf_topk", tabA, idxA, tabB, idxB, packed, k, seen, True, (gmfA, gmfB, w))


def neumf_rank(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], gmfA: torch.Tensor,
               gmfB: torch.Tensor, packed: PackedMLP, w: torch.Tensor, targets: tuple, max_targets: int, seen: Optional[tuple] = None,
               rank: Optional[torch.Tensor] = None):
    """ncf_neumf_rank: exactly ``rank_rows(neumf_score over every (user, item) pair, targets, seen)``; as mlp_rank otherwise, and
    ``ranking_plan("mlp_rank", ...)`` is its plan."""
    return _mlp_rank("neumf_rank", tabA, idxA, tabB, idxB, packed, targets, max_targets, seen, True, rank, (gmfA, gmfB, w))


# ncf_ranking_plan's entry (include/ncf_abi.h enum ncf_ranking_entry)
RANKING_ENTRIES = {"topk_rows": 0, "rank_rows": 1, "dot_topk": 2, "dot_rank": 3, "mlp_topk": 4, "mlp_rank": 5}


def ranking_plan(entry: str, rows: int, cols: int, k_or_max_targets: int = 1):
    """(tile_cols, tiles, merge_levels, chunk_rows) of the launch the ranking entry point ``entry`` (a key of RANKING_ENTRIES) picks
    for (rows, cols) and its k (top-K entries) or max_targets (rank entries): columns per workgroup tile / wave range, tiles per
    row, merge launches after the first level and rows per pass over the key workspace (rank entries: 0 and rows).  The entry
    point's own refusals raise NativeError.  Host only: no launch, no device."""
    return _query(load_library().ncf_ranking_plan, (RANKING_ENTRIES[entry], int(rows), int(cols), int(k_or_max_targets)),
                  (_c_int, _c_i64, _c_int, _c_i64))


# ------------------------------------------------------------------ full-catalogue softmax loss of a dot-product readout
# ncf_dot_softmax_plan's kind (include/ncf_abi.h enum ncf_dot_softmax_kind)
DOT_SOFTMAX_KINDS = {"lse": 0, "grad_rows": 1, "grad_items": 2}
DOT_SOFTMAX_MAX_ROWS = 65536        # listed rows per call (include/ncf_abi.h: rows <= 65536); more is NCF_EUNSUPPORTED


def dot_softmax_plan(kind: str, rows: int, cols: int, D: int):
    """(tile, tiles, chunk_rows) of the launch ``dot_lse`` (kind "lse") or one role of ``dot_softmax_grad`` ("grad_rows": the batch
    rows walk the catalogue; "grad_items": the catalogue's rows walk the batch) picks for a (rows, cols) problem of width D: the
    walk's tile, its number of tiles, and the resident rows per pass over the partial-output workspace.  Host only."""
    return _query(load_library().ncf_dot_softmax_plan, (DOT_SOFTMAX_KINDS[kind], int(rows), int(cols), int(D)), (_c_i64, _c_i64, _c_i64))


def dot_lse(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor], scale: float = 1.0,
            return_max: bool = False):
    """ncf_dot_lse: ``lse`` (B,) fp32, the log-sum-exp over every column c of the list idxB (every row of tabB with idxB None) of
    ``scale * <tabA[idxA[b]], tabB[idxB[c]]>`` (operands as dot_topk; the score bits are gather_dot's), without the B x I logit
    matrix.  ``return_max``: (lse, max logit per row, exact).  Output and workspace from the caching allocator on the current
    stream; no sync.  An id outside its table sets the sticky flag check_oob reads."""
    lib = load_library()
    args, (B, I, D, dev) = _dot_operands("dot_lse", tabA, idxA, tabB, idxB)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    mx = torch.empty(B, dtype=torch.float32, device=dev) if return_max else None
    nbytes = lib.ncf_dot_lse_workspace_bytes(B, I, D)
    ws = _workspace(nbytes, dev)
    _check(lib.ncf_dot_lse(*args, float(scale), _ptr(lse), _ptr(mx), _ptr(ws), nbytes, _ptr(_oob_flag(dev)), _stream(tabA)))
    return (lse, mx) if return_max else lse


def dot_softmax_grad(tabA: torch.Tensor, idxA: Optional[torch.Tensor], tabB: torch.Tensor, idxB: Optional[torch.Tensor],
                     targets: torch.Tensor, lse: torch.Tensor, g: torch.Tensor, scale: float = 1.0, need=(True, True)):
    """ncf_dot_softmax_grad in both roles: ``(dA_rows (B, D), dQ (I, D))``, the gradients of ``sum_b g[b] * (lse[b] - z[b, targets[b]])``
    (``lse`` from dot_lse with the same operands and scale) by the listed rows (one gradient row per LISTED row) and by the
    columns of the list.  ``targets`` (B,) int64 columns of the list, ``lse`` / ``g`` (B,) fp32.  ``need``: a role that is False
    is not run and returns None.  Each role takes its own workspace from the caching allocator; deterministic; no sync."""
    lib = load_library()
    who = "dot_softmax_grad"
    args, (B, I, D, dev) = _dot_operands(who, tabA, idxA, tabB, idxB)
    _vec1d(who, targets, "targets", torch.int64, B)
    _vec1d(who, lse, "lse", torch.float32, B)
    _vec1d(who, g, "g", torch.float32, B)
    _dev_all((targets, "targets"), (lse, "lse"), (g, "g"))
    outs = []
    for items, rows_out in ((0, B), (1, I)):
        if not need[items]:
            outs.append(None)
            continue
        out = torch.empty((rows_out, D), dtype=torch.float32, device=dev)
        nbytes = lib.ncf_dot_softmax_grad_workspace_bytes(B, I, D, items)
        ws = _workspace(nbytes, dev)
        _check(lib.ncf_dot_softmax_grad(*args, _ptr(targets), _ptr(lse), _ptr(g), float(scale), items, _ptr(out), _ptr(ws), nbytes,
                                        _ptr(_oob_flag(dev)), _stream(tabA)))
        del ws
        outs.append(out)
    return tuple(outs)
