// What the fused dot-product entry points share (dot_topk.hip: ncf_dot_topk; rank.hip: ncf_dot_rank).  Device: the wave shape and
// the MFMA operand loads of the scoring half; what a kernel does with the scores (candidate buffer and threshold, or rank
// counters) is its own, and so is its copy of the column walk (DESIGN.md 4.22 says why).  Host: the column tiling, the number of
// MFMA steps and the dispatch over it, and the width / size / operand refusals.  See dot_topk.hip for the chain layout that makes
// a score gather_dot_kernel<false>'s bit for bit.
// Internal: not part of the ABI.
#pragma once
#include "topk_common.h"

namespace ncf {

constexpr int kDtWaves = 4;
constexpr int kDtThreads = kDtWaves * kWave;
constexpr int kDtUsers = 16;                       // users per wave (the MFMA M dimension)
constexpr int kDtBlockUsers = kDtWaves * kDtUsers; // users per workgroup
constexpr int kDtMaxD = 256;                       // fused limit on the embedding width (user rows live in registers)
constexpr int kDtChunk = 2048;                     // columns per exclusion bitmap
constexpr int kDtKS = 4;                           // chain elements per MFMA step (the instruction's K)
constexpr int64_t kDtTargetBlocks = 512;           // tile_cols shrinks (8192 -> 2048) until the grid reaches this

// 16 floats of a row starting at element e0 (elements >= D read as 0)
__device__ __forceinline__ void load_block(const float* __restrict__ row, int e0, int D, bool vec, float (&v)[16]) {
    if (vec && e0 + 16 <= D) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(row + e0 + 4 * h);
            v[4 * h] = q[0]; v[4 * h + 1] = q[1]; v[4 * h + 2] = q[2]; v[4 * h + 3] = q[3];
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) v[s] = e0 + s < D ? row[e0 + s] : 0.f;
    }
}

// J steps of kDtKS chain elements: lane (row l & 15, slot q = l >> 4) holds block kDtKS j + q of its row (zeros past D / q >= kDtKS)
template <int J>
__device__ __forceinline__ void load_frag(const float* row, int D, bool vec, int q, float (&v)[J][16]) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (row && q < kDtKS) load_block(row, 16 * (kDtKS * j + q), D, vec, v[j]);
        else {
#pragma unroll
            for (int s = 0; s < 16; ++s) v[j][s] = 0.f;
        }
    }
}

// The fused level's column tiles: tile_cols shrinks (8192 -> kDtChunk) until the grid reaches kDtTargetBlocks
inline int dot_topk_tile_cols(int64_t rows, int64_t cols) {
    const int64_t ublocks = (rows + kDtBlockUsers - 1) / kDtBlockUsers;
    int tile_cols = kTopkTile;
    while (tile_cols > kDtChunk && ublocks * ((cols + tile_cols - 1) / tile_cols) < kDtTargetBlocks) tile_cols >>= 1;
    return tile_cols;
}

// ---- host side shared by the two entry points; `what` names the entry point in the error string ----

// MFMA steps over a width: the J of the kernel instance
inline int dot_steps(int D) { return (D + 16 * kDtKS - 1) / (16 * kDtKS); }

// LAUNCH(J) for the instance that covers `steps` (1 .. 4: D <= kDtMaxD)
#define NCF_DOT_DISPATCH(steps, LAUNCH) \
    switch (steps) {                    \
        case 1: LAUNCH(1); break;       \
        case 2: LAUNCH(2); break;       \
        case 3: LAUNCH(3); break;       \
        default: LAUNCH(4); break;      \
    }

// the width and size refusals, made after the entry point's own limit (k or max_targets)
inline int dot_check_shape(const char* what, int64_t rows, int64_t cols, int D) {
    if (D < 1 || D > kDtMaxD) return fail(NCF_EUNSUPPORTED, "%s: width D = %d is outside the fused range 1 .. %d", what, D, kDtMaxD);
    return topk_check_size(what, rows, cols);
}

// ncf_dot_topk's refusal on k and its merge plan (dot_topk.hip), also answered by ncf_ranking_plan (rank.hip)
int dot_topk_check_k(const char* what, int k);
TopkMerge dot_topk_plan(int64_t rows, int64_t cols, int tile_cols, int k);

// the operand refusals of a call with rows > 0.  outputs: the caller's output pointers that share the "null argument" refusal are all there
inline int dot_check_operands(const char* what, const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                              const int64_t* idxA, const int64_t* idxB, int64_t rows, int64_t cols, int D, bool outputs) {
    if (!tabA || !tabB || !outputs) return fail(NCF_EINVAL, "%s: null argument", what);
    if (ldA < D || ldB < D) return fail(NCF_EINVAL, "%s: leading dimension smaller than D = %d", what, D);
    if (!idxA && rows > rowsA) return fail(NCF_EINVAL, "%s: rows = %lld > rowsA without idxA", what, (long long)rows);
    if (!idxB && cols > rowsB) return fail(NCF_EINVAL, "%s: cols = %lld > rowsB without idxB", what, (long long)cols);
    return NCF_OK;
}

}  // namespace ncf
