// Shared pieces of the exact-rank entry points (rank.hip: ncf_rank_rows, ncf_dot_rank; mlp_topk.hip: ncf_mlp_rank).
//
// Contract: rank[t] of a target column is the number of non-excluded columns of its row whose key (topk_common.h:
// map(score) << 32 | ~column) is greater than the target's, i.e. the slot the target would hold in an unbounded ncf_topk_rows
// result; -1 for a target that is excluded or outside [0, cols).  ranked[r] is the number of non-excluded columns of row r.
//
// Shape shared by the three: a preparation kernel turns each row's targets into keys, sorted ascending in chunks of `cap` entries
// (skey, with sperm = the entry's place inside its chunk), and initialises rank (0, or -1 for an invalid target, whose key is
// kRankNoKey and sorts last).  A counting kernel then streams the columns; for each non-excluded column key x it finds
// p = #{chunk keys < x} and bumps hist[p] in LDS: x beats exactly the targets in slots 0 .. p-1, so after the tile the count of
// slot j is the suffix sum hist[j+1] + ... + hist[P].  Each (row, tile) adds its counts into rank / ranked with int32 atomics:
// integer sums, so the result does not depend on the order the tiles finish in.  A row with one target keeps the key in a
// register and a private counter instead (the leave-one-out form).
// Here: the key, the LDS chunk helpers of the counting kernels, and the host steps of every rank call (workspace, target refusals,
// expand, prepare).  What a fused rank call shares with its top-K sibling (operand refusals, tiling, dispatch) lives with the
// scorer: dot_frag.h for the dot pair, mlp_topk.hip for the MLP pair.
// Internal: not part of the ABI.
#pragma once
#include "topk_common.h"

namespace ncf {

constexpr int kRankMaxTargets = 128;                   // targets per row of a fused call; chunk of ncf_rank_rows
constexpr unsigned long long kRankNoKey = ~0ull;       // no valid key has map(score) = 0xFFFFFFFF (that pattern is a NaN's: it maps to 0)

__device__ __forceinline__ unsigned long long rank_key(float score, int64_t col) {
    return ((unsigned long long)topk_map(score) << 32) | (0xFFFFFFFFu - (uint32_t)col);
}

// slots of a target chunk in LDS: max_targets rounded up to a power of two (>= 2)
inline int rank_slots(int max_targets) {
    int P = 2;
    while (P < max_targets) P <<= 1;
    return P;
}

// #{keys[0 .. P) < x} for ascending keys padded with kRankNoKey to P slots (P a power of two): log2(P) + 1 reads, no branch
__device__ __forceinline__ int rank_lower_bound(const unsigned long long* keys, int P, unsigned long long x) {
    int pos = 0;
    for (int s = P >> 1; s >= 1; s >>= 1)
        if (keys[pos + s - 1] < x) pos += s;
    return pos + (keys[pos] < x ? 1 : 0);
}

// threads tid, tid + nt, ...: the chunk's n sorted keys into keys[0 .. P) (padded) and hist[0 .. P] = 0.  The caller orders LDS after it.
__device__ __forceinline__ void rank_stage(unsigned long long* keys, uint32_t* hist, const unsigned long long* __restrict__ src, int n,
                                           int P, int tid, int nt) {
    for (int s = tid; s < P; s += nt) keys[s] = s < n ? src[s] : kRankNoKey;
    for (int s = tid; s <= P; s += nt) hist[s] = 0u;
}

// one thread: hist[p] <- hist[p] + ... + hist[P]; the count of slot j is then hist[j + 1]
__device__ __forceinline__ void rank_suffix(uint32_t* hist, int P) {
    uint32_t run = 0;
    for (int p = P; p >= 1; --p) {
        run += hist[p];
        hist[p] = run;
    }
}

// threads tid, tid + nt, ...: add each valid slot's count to its entry of rank (rank_chunk = the chunk's first entry)
__device__ __forceinline__ void rank_flush(const unsigned long long* keys, const uint32_t* hist, const int32_t* __restrict__ perm, int n,
                                           int32_t* rank_chunk, int tid, int nt) {
    for (int s = tid; s < n; s += nt) {
        const uint32_t c = hist[s + 1];
        if (c && keys[s] != kRankNoKey) atomicAdd(rank_chunk + perm[s], (int)c);
    }
}

// ---- host side, defined in rank.hip ----

// workspace of a rank call over n_targets target entries: sorted keys + places; fused: + the (user, item) ids and scores of the
// (row, target) pairs for the pair scorer
struct RankWs {
    unsigned long long* skey;
    int32_t* sperm;
    int64_t* pair_user;
    int64_t* pair_item;
    float* pair_score;
};
size_t rank_ws_bytes(int64_t n_targets, bool fused);
RankWs rank_ws_carve(void* workspace, int64_t n_targets, bool fused);

// refusals shared by the three entry points (after topk_check_size)
int rank_check_args(const char* what, const char* query, int64_t rows, const int64_t* seen_rowptr, const int32_t* seen_col,
                    const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, const int32_t* rank, const int32_t* ranked,
                    const void* workspace, size_t workspace_bytes, size_t need);
int rank_check_max_targets(const char* what, int max_targets);

// fused calls, step 1: ranked <- 0 and the pair ids of every (row, target) entry (out-of-range target columns take item id 0: their
// score is never used)
void rank_expand(const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, const int64_t* tgt_rowptr,
                 const int32_t* tgt_col, int64_t n_targets, const RankWs& w, int32_t* ranked, hipStream_t s);
// step 2 (after the pair scorer; step 1 of ncf_rank_rows with scores given): keys, order, rank <- 0 / -1.  single: one chunk of
// `cap` entries per row, the rest -1 and *overflow = 1.
void rank_prepare(const float* scores, int64_t ld, const float* pair_score, int64_t rows, int64_t cols, const int64_t* seen_rowptr,
                  const int32_t* seen_col, const int64_t* tgt_rowptr, const int32_t* tgt_col, int cap, bool single, const RankWs& w,
                  int32_t* rank, int32_t* overflow, hipStream_t s);

// ncf_ranking_plan's answer for ncf_mlp_topk (rank = false: tile_cols and the merge plan) and ncf_mlp_rank (tile_cols), after the
// entry point's own limit and size refusals; defined beside the launches in mlp_topk.hip
int mlp_ranking_plan(bool rank, int64_t rows, int64_t cols, int k_or_max_targets, const char* what, int* tile_cols, TopkMerge* merge);

}  // namespace ncf
