// Shared pieces of the per-row top-K (topk.hip: ncf_topk_rows; dot_topk.hip: ncf_dot_topk; mlp_topk.hip: ncf_mlp_topk): the key
// map, the wave-wide candidate helpers of the fused kernels, and the host API of the merge levels (plan, workspace, launches,
// shared refusals), which topk.hip defines together with the tile select kernel they run.  See topk.hip for the ordering
// contract and the kernel shape.  Internal: not part of the ABI.
#pragma once
#include "ncf_common.h"

namespace ncf {

constexpr int kTopkThreads = 256;
constexpr int kTopkTile = 8192;                        // entries per workgroup: 32 per thread
constexpr int kTopkPer = kTopkTile / kTopkThreads;
constexpr int kTopkMaxK = 1024;
constexpr int64_t kTopkMaxCols = int64_t(1) << 24;
constexpr int64_t kTopkMaxRows = 65536;
constexpr size_t kTopkChunkBytes = size_t(256) << 20;  // workspace target: rows are processed in chunks that fit it

__device__ __forceinline__ uint32_t topk_map(float x) {
    uint32_t u = __float_as_uint(x);
    if (x != x) return 0u;                              // every NaN: below -inf
    if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inverse of topk_map for every key that is not a NaN's (0 maps back to a NaN); -0.0 comes back as +0.0
__device__ __forceinline__ float topk_unmap(uint32_t m) {
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((int)(uint32_t)v, m), hi = __shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

// (key >> top) == (ref >> top), with top = 64 meaning "no bits": true
__device__ __forceinline__ bool topk_high_eq(unsigned long long key, unsigned long long ref, int top) {
    return top >= 64 || ((key ^ ref) >> top) == 0;
}

// order this wave's LDS accesses (the LDS serves one wave's instructions in order; the fence keeps the compiler from moving
// memory operations across it)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// The largest key T with #{v >= T} >= keep over the wave's 4 x 64 keys (0 = empty; at least `keep` nonzero keys present).
__device__ unsigned long long wave_kth(const unsigned long long (&v)[4], int keep) {
    unsigned long long prefix = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = prefix | (1ull << bit);
        int c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) c += __popcll(__ballot(v[i] >= cand));
        if (c < keep) continue;
        prefix = cand;
        if (c == keep) {                 // exactly `keep` keys are >= cand: the smallest of them is the answer
            unsigned long long m = ~0ull;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v[i] >= cand) m = min(m, v[i]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = min(m, shfl_xor_u64(m, o));
            return m;
        }
    }
    return prefix;
}

// keep the `keep` best of the wave's n candidate keys buf[0 .. n) (n <= 4 x 64), compacted to the front; returns the keep-th key.
// The caller orders the wave's LDS accesses around it (wave_lds_sync) and keeps its own count and threshold.
__device__ unsigned long long wave_reselect(unsigned long long* buf, int n, int keep, int lane) {
    unsigned long long v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lane + 64 * i < n ? buf[lane + 64 * i] : 0ull;
    const unsigned long long kth = wave_kth(v, keep);
    wave_lds_sync();
    int base = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool f = v[i] != 0ull && v[i] >= kth;
        const unsigned long long m = __ballot(f);
        if (f) *(buf + lanes_below(m) + base) = v[i];   // this operand order keeps the fused kernels' address code as it was
        base += __popcll(m);
    }
    return kth;
}

// ---- host side, defined in topk.hip: the merge levels every top-K entry point ends with ----

constexpr int topk_kp(int k) { return (k + 1) & ~1; }   // key slots per tile: k rounded up to even (16-byte aligned pairs)

// The merge plan of one row.  Its first level (ncf_topk_rows' level 0 or a fused score-and-select kernel) writes n1 keys per row
// (kp per tile) into buffer A; each merge level runs topk_tile_kernel over kp keys per tile of the previous level until one tile
// is left, ping-ponging between A and B.  n1 = 0: the first level finishes alone (no merge, no workspace).
struct TopkMerge {
    int kp;
    int levels;              // merge launches (the last one sorts and writes the result)
    int64_t tiles[8];        // tiles per merge level
    int64_t n1, n2;          // keys per row in the two ping-pong buffers
    int64_t chunk;           // rows per chunk: the buffers stay near kTopkChunkBytes
};

// align > 1: a chunk of more than `align` rows that does not take every row is rounded down to a multiple of `align`
TopkMerge topk_merge_plan(int64_t rows, int64_t n1, int k, int64_t align = 1);
size_t topk_merge_bytes(const TopkMerge& p);
// ncf_topk_rows' plan: level 0 over the columns, then the merge levels (n1 = 0 for a row of one tile)
TopkMerge topk_rows_plan(int64_t rows, int64_t cols, int k);
// The merge levels of rows [r0, r0 + nr) (local row 0 of buffer A = row r0).  scores / ld: the final level re-reads each
// score from the caller's matrix; null: it recovers the score from the key.
void topk_merge(const TopkMerge& p, unsigned long long* bufA, const float* scores, int64_t ld, int64_t r0, int64_t nr, int k,
                float* out_score, int32_t* out_idx, int32_t* out_count, hipStream_t s);

// The refusals every entry point shares, in the order each one makes them; `what` names the entry point in the error string.
int topk_check_k(const char* what, int k, int fused_max_k);       // fused_max_k = kTopkMaxK: no fused limit
int topk_check_size(const char* what, int64_t rows, int64_t cols);
int topk_check_buffers(const char* what, const char* query, const int64_t* seen_rowptr, const int32_t* seen_col, const void* workspace,
                       size_t workspace_bytes, size_t need);

}  // namespace ncf
