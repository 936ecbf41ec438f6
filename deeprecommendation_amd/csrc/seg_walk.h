// The segment walk of the graph kernels (spmm.hip, edge_softmax.hip, gat.hip, edge_keep.hip): one wave owns one SEGMENT of a prepared
// CSR (a contiguous entry range of one row, at most seg_len long; without a `row_of` map the segments are the rows), four waves to
// a block, waves striding over the segments.  Every piece of that walk is stated here once.
#pragma once
#include "ncf_common.h"
#include <math.h>
#include <type_traits>

namespace ncf {

// ---- which segments a wave owns: const WaveWalk walk = wave_walk(blockDim.x); for (s = walk.first; s < n; s += walk.stride).
// The kernel reads its own blockDim.x: only inside a kernel does the compiler know that every block has the full size, and a read
// from a helper costs a remainder check and a vector load.
struct WaveWalk { int64_t first, stride; };
__device__ __forceinline__ WaveWalk wave_walk(unsigned block_threads) {
    return WaveWalk{(int64_t)blockIdx.x * (block_threads >> 6) + (threadIdx.x >> 6), (int64_t)gridDim.x * (block_threads >> 6)};
}

// blocks of 256 threads for one wave per item, capped: the waves stride over what is left
inline unsigned wave_blocks(int64_t n) {
    int64_t b = (n + 3) / 4;
    if (b > 256 * 64) b = 256 * 64;
    return (unsigned)b;
}

// ---- the row of a segment, and whether the segment opens / closes its row.  A segment that does both holds the whole row and
// writes the result; any other writes its partial sum for the next level.  Without a map (row_of == NULL) every segment is a row;
// HAS_MAP: the caller has already read row_of, so the test for NULL is left out.
__device__ __forceinline__ int64_t seg_row(const int32_t* __restrict__ row_of, int64_t s) { return row_of ? (int64_t)row_of[s] : s; }
template <bool HAS_MAP = false, typename R>
__device__ __forceinline__ bool seg_opens_row(const int32_t* __restrict__ row_of, int64_t s, R row) {
    if (HAS_MAP) return s == 0 || row_of[s - 1] != row;
    return !row_of || s == 0 || row_of[s - 1] != row;
}
template <bool HAS_MAP = false, typename R>
__device__ __forceinline__ bool seg_closes_row(const int32_t* __restrict__ row_of, int64_t s, int64_t n_seg, R row) {
    if (HAS_MAP) return s == n_seg - 1 || row_of[s + 1] != row;
    return !row_of || s == n_seg - 1 || row_of[s + 1] != row;
}

// ---- 64-lane butterflies, offsets 32 down to 1: every lane ends with the result, in one fixed order.  gat_row_sum_kernel and
// gat_reduce_kernel spell the sum out instead: through the helper the compiler schedules them differently.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- lane layout of the row-gathering kernels: LPR = D/4 lanes (rounded up to a power of two) own one row's 16-byte chunks, so a
// wave-instruction reads EPI = 64/LPR whole rows; UNROLL such instructions are kept in flight per lane.  A lane whose chunk is not
// below the row's chunk count is idle.
template <int LPR>
struct RowLanes {
    static constexpr int EPI = 64 / LPR;  // entries per wave-instruction
    static constexpr int UNROLL = 4;
    static __device__ __forceinline__ int chunk(int lane) { return lane % LPR; }   // 16-byte chunk of the row this lane owns
    static __device__ __forceinline__ int entry(int lane) { return lane / LPR; }   // which of the EPI concurrent entries
};

// f(std::integral_constant<int, LPR>) for the LPR that covers `chunks` 16-byte chunks (chunks <= 64)
template <typename F>
inline void dispatch_lpr(int chunks, F&& f) {
    if (chunks <= 8) f(std::integral_constant<int, 8>{});
    else if (chunks <= 16) f(std::integral_constant<int, 16>{});
    else if (chunks <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

}  // namespace ncf
