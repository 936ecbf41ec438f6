// Which edges one GraphNCF training step keeps (include/ncf_abi.h, "THE KEEP RULE"): the batch's target edges, node dropout and
// message dropout applied in one pass over the CSR by destination, with the degrees of the remaining edges counted on the way.
//
// A streaming pass, about 24 bytes per entry (col 4, pair_key 8, slot 4, attr 4 read; w_out 4 written).  One wave owns one level-0
// SEGMENT of the prepared CSR (at most seg_len consecutive entries of one destination row), so every per-entry array is read and
// written with 64 consecutive elements per wave-instruction.  The node mask (N bytes) and the sorted targets (8 B per batch pair)
// are small next to the entry arrays and stay in cache; the target lookup is a per-lane binary search.  The kept entries of a
// segment are counted across the wave and lane 0 adds the count to deg_out[row] with one INTEGER atomic add: integer sums do not
// depend on arrival order, so the degrees (and with them every coefficient) are bitwise reproducible.  No MFMA, no LDS.
#include "ncf_common.h"
#include "drop_mask.h"   // drop_threshold: the one drop rule
#include "seg_walk.h"    // wave_walk / wave_blocks, seg_row, wave_sum
#include <math.h>

namespace ncf {

// true iff key occurs in sorted[0 .. n): lower bound by bisection, n >= 1
__device__ __forceinline__ bool among_sorted(const int64_t* __restrict__ sorted, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == key;
}

__global__ __launch_bounds__(256) void edge_keep_kernel(const int64_t* __restrict__ segptr, const int32_t* __restrict__ row_of,
                                                        int64_t n_seg, int64_t N, const int32_t* __restrict__ col,
                                                        const float* __restrict__ attr, const int64_t* __restrict__ pair_key,
                                                        const int64_t* __restrict__ targets, int64_t n_targets,
                                                        const int32_t* __restrict__ slot, uint32_t thr, uint32_t seed,
                                                        const uint8_t* __restrict__ node_keep, float* __restrict__ w_out,
                                                        int32_t* __restrict__ deg_out) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t s = walk.first; s < n_seg; s += walk.stride) {
        const int64_t beg = segptr[s], end = segptr[s + 1];
        const int64_t row = seg_row(row_of, s);
        const bool row_ok = row >= 0 && row < N;
        const bool dst_kept = row_ok && (!node_keep || node_keep[row] != 0);
        int cnt = 0;
        for (int64_t e = beg + lane; e < end; e += kWave) {
            bool kept = dst_kept;
            if (node_keep) {
                const int64_t src = col[e];
                kept = kept && src >= 0 && src < N && node_keep[src] != 0;
            }
            if (thr) kept = kept && (mix32((uint32_t)slot[e] * 0x9E3779B1U ^ seed) >> 16) >= thr;
            if (kept && n_targets > 0) kept = !among_sorted(targets, n_targets, pair_key[e]);
            w_out[e] = kept ? (attr ? attr[e] : 1.f) : 0.f;
            cnt += kept ? 1 : 0;
        }
        cnt = wave_sum(cnt);
        if (lane == 0 && cnt > 0 && row_ok) atomicAdd(deg_out + row, cnt);
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_edge_keep(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, int64_t N, const int32_t* col,
                             const float* attr, const int64_t* pair_key, const int64_t* targets_sorted, int64_t n_targets,
                             const int32_t* slot, float p, uint32_t seed, const uint8_t* node_keep, float* w_out, int32_t* deg_out,
                             ncf_stream_t stream) {
    if (n_seg < 0 || N < 0 || n_targets < 0) return fail(NCF_EINVAL, "ncf_edge_keep: negative size");
    if (!isfinite(p) || !(p >= 0.f && p <= 1.f)) return fail(NCF_EINVAL, "ncf_edge_keep: p = %g is not in [0, 1]", (double)p);
    const uint32_t thr = drop_threshold(p).thr;
    if (!segptr || (N > 0 && !deg_out) || (n_seg > 0 && (!col || !w_out))) return fail(NCF_EINVAL, "ncf_edge_keep: null pointer");
    if (n_targets > 0 && (!pair_key || !targets_sorted)) return fail(NCF_EINVAL, "ncf_edge_keep: target masking needs pair_key and the sorted targets");
    if (thr > 0 && !slot) return fail(NCF_EINVAL, "ncf_edge_keep: message dropout (thr = %u) needs the per-entry slot", thr);
    hipStream_t s = (hipStream_t)stream;
    fill_u32_async(deg_out, 0u, (size_t)N * sizeof(int32_t), s);
    if (n_seg > 0)
        hipLaunchKernelGGL(edge_keep_kernel, dim3(wave_blocks(n_seg)), dim3(256), 0, s, segptr, row_of, n_seg, N, col, attr, pair_key,
                           targets_sorted, n_targets, slot, thr, seed, node_keep, w_out, deg_out);
    return check_launch("ncf_edge_keep");
}
