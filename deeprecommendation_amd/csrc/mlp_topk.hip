// ncf_mlp_topk and ncf_mlp_rank: the MLP readout's instances of the full-catalogue kernels and entry bodies of mlp_topk.h (which has
// the design), and what ncf_ranking_plan answers for them.  neumf.hip instantiates the same header with the GMF term on.
#include "mlp_topk.h"

namespace ncf {

// what ncf_ranking_plan (rank.hip) answers for the two MLP entry points: the entry's refusals, then the functions its launch calls
int mlp_ranking_plan(bool rank, int64_t rows, int64_t cols, int k_or_max_targets, const char* what, int* tile_cols, TopkMerge* merge) {
    if (rank) {
        if (const int rc = mr_check(rows, cols, k_or_max_targets, what)) return rc;
        *tile_cols = mr_tile_cols(rows, cols, k_or_max_targets);
        return NCF_OK;
    }
    if (const int rc = mt_check(rows, cols, k_or_max_targets, what)) return rc;
    *merge = mt_plan(rows, cols, k_or_max_targets, tile_cols);
    return NCF_OK;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_mlp_topk_supported(int dtype, int EA, int EB, int n_layers, const int* dims, int k) {
    return (mt_shape_ok(dtype, EA, EB, n_layers, dims) && k >= 1 && k <= kMtMaxK) ? 1 : 0;
}

extern "C" size_t ncf_mlp_topk_workspace_bytes(int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims, int k) {
    return mlp_topk_ws_bytes("ncf_mlp_topk_workspace_bytes", MlpNoGmf(), rows, cols, user_first, n_layers, dims, k);
}

extern "C" int ncf_mlp_topk(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB,
                            int EA, int EB, int user_first, const int64_t* user_ids, const int64_t* item_ids, int64_t rows,
                            int64_t cols, int n_layers, const int* dims, const void* packed, const int64_t* seen_rowptr,
                            const int32_t* seen_col, int k, float* out_score, int32_t* out_idx, int32_t* out_count, void* workspace,
                            size_t workspace_bytes, int32_t* oob, ncf_stream_t stream) {
    return mlp_topk_run("ncf_mlp_topk", "ncf_mlp_topk_workspace_bytes", MlpNoGmf(), dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, EA, EB,
                        user_first, user_ids, item_ids, rows, cols, n_layers, dims, packed, seen_rowptr, seen_col, k, out_score, out_idx,
                        out_count, workspace, workspace_bytes, oob, (hipStream_t)stream);
}

extern "C" int ncf_mlp_rank_supported(int dtype, int EA, int EB, int n_layers, const int* dims, int max_targets) {
    return (mt_shape_ok(dtype, EA, EB, n_layers, dims) && max_targets >= 1 && max_targets <= kRankMaxTargets) ? 1 : 0;
}

extern "C" size_t ncf_mlp_rank_workspace_bytes(int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims, int64_t n_targets,
                                               int max_targets) {
    return mlp_rank_ws_bytes("ncf_mlp_rank_workspace_bytes", MlpNoGmf(), rows, cols, user_first, n_layers, dims, n_targets, max_targets);
}

extern "C" int ncf_mlp_rank(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB,
                            int EA, int EB, int user_first, const int64_t* user_ids, const int64_t* item_ids, int64_t rows,
                            int64_t cols, int n_layers, const int* dims, const void* packed, const int64_t* seen_rowptr,
                            const int32_t* seen_col, const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, int max_targets,
                            int32_t* rank, int32_t* ranked, void* workspace, size_t workspace_bytes, int32_t* oob, int32_t* overflow,
                            ncf_stream_t stream) {
    // the targets' own scores: ncf_score_fused over the (row, target) pairs, the first part's ids first
    auto score_pairs = [&](const int64_t* users, const int64_t* items, int64_t n, float* out) {
        return ncf_score_fused(dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, user_first ? users : items, user_first ? items : users, n, EA, EB,
                               n_layers, dims, packed, out, oob, stream);
    };
    return mlp_rank_run("ncf_mlp_rank", "ncf_mlp_rank_workspace_bytes", MlpNoGmf(), score_pairs, dtype, tabA, rowsA, ldA, tabB, rowsB, ldB,
                        EA, EB, user_first, user_ids, item_ids, rows, cols, n_layers, dims, packed, seen_rowptr, seen_col, tgt_rowptr, tgt_col,
                        n_targets, max_targets, rank, ranked, workspace, workspace_bytes, oob, overflow, (hipStream_t)stream);
}
