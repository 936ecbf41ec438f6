// Per-row top-K with an exclusion list (ncf_topk_rows): the ranking step behind a recommendation request — the reference sorts
// the whole score vector on the host (webapp/backend.py:78-121: DataFrame.sort_values(...).iloc[:k]); here only k (score, id)
// pairs per row leave the device.
//
// Order: every candidate carries a 64-bit key  (map(score) << 32) | (0xFFFFFFFF - col)  where map() is the order-preserving
// fp32 -> uint32 map with -0.0 folded onto +0.0 and every NaN mapped to 0 (below -inf, which maps to 0x007FFFFF).  Keys are unique
// within a row (the column is part of it), so "the k largest keys" is exactly torch.sort(descending, stable) after the excluded
// columns are removed: equal scores go to the lower column first, NaNs last and by column.  Key 0 means "no candidate".
//
// Shape: a row is cut into tiles of kTile = 8192 entries, one 256-thread workgroup per tile, 32 keys per thread in registers.
//   level 0   reads scores (16-byte loads where aligned), applies the exclusion list through an LDS bitmap of the excluded ids that
//             fall inside the tile, and selects the tile's k best keys;
//   level >0  reads the previous level's candidate keys (kp = k rounded up to even slots per tile, 0-padded) in tiles of the
//             same size and selects again.
// A row that fits one tile is done in one launch; a longer row takes as many levels as it needs to reach one tile (each level
// divides its length by >= 8: 2^20 columns take three launches at k = 100 and four at k = 1024, 2^24 at k = 1024 five).  The last level sorts its
// survivors in LDS (bitonic) and writes (score, column) pairs, the score re-read from the input so its bits are the caller's.
// Selection inside a tile is a radix select on the keys with per-wave LDS histograms (4 x 256 bins): the first digit starts at
// the highest bit in which the tile's valid keys differ (found by a min / max reduction), so the common high bits of a narrow
// score range cost no pass; a pass ends the select as soon as the bucket that holds the k-th key is taken whole.
#include "topk_common.h"

using namespace ncf;

extern "C" size_t ncf_topk_workspace_bytes(int64_t rows, int64_t cols, int k) {
    if (!topk_shape_ok(rows, cols, k) || rows == 0) return 0;
    const TopkPlan p = topk_plan(rows, cols, k);
    return (size_t)(p.chunk * (p.n1 + p.n2) * 8);
}

extern "C" int ncf_topk_rows(const float* scores, int64_t rows, int64_t cols, int64_t ld, const int64_t* seen_rowptr, const int32_t* seen_col,
                             int k, float* out_score, int32_t* out_idx, int32_t* out_count, void* workspace, size_t workspace_bytes,
                             ncf_stream_t stream) {
    if (k < 1 || k > kTopkMaxK) return fail(NCF_EINVAL, "ncf_topk_rows: k = %d is outside 1 .. %d", k, kTopkMaxK);
    if (cols < 1 || cols > kTopkMaxCols)
        return fail(NCF_EUNSUPPORTED, "ncf_topk_rows: cols = %lld is outside 1 .. %lld", (long long)cols, (long long)kTopkMaxCols);
    if (rows < 0 || rows > kTopkMaxRows)
        return fail(NCF_EUNSUPPORTED, "ncf_topk_rows: rows = %lld is outside 0 .. %lld", (long long)rows, (long long)kTopkMaxRows);
    if (ld < cols) return fail(NCF_EINVAL, "ncf_topk_rows: ld = %lld < cols = %lld", (long long)ld, (long long)cols);
    if (rows == 0) return NCF_OK;
    if (!scores || !out_score || !out_idx || !out_count) return fail(NCF_EINVAL, "ncf_topk_rows: null argument");
    if ((seen_rowptr == nullptr) != (seen_col == nullptr))
        return fail(NCF_EINVAL, "ncf_topk_rows: seen_rowptr and seen_col are given together or not at all");
    const TopkPlan p = topk_plan(rows, cols, k);
    const size_t need = (size_t)(p.chunk * (p.n1 + p.n2) * 8);
    if (workspace_bytes < need)
        return fail(NCF_EWORKSPACE, "ncf_topk_rows: workspace of %zu bytes, %zu needed (ncf_topk_workspace_bytes)", workspace_bytes, need);
    if (need && (!workspace || !aligned16(workspace))) return fail(NCF_EINVAL, "ncf_topk_rows: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* bufA = (unsigned long long*)workspace;
    unsigned long long* bufB = bufA + p.chunk * p.n1;
    for (int64_t r0 = 0; r0 < rows; r0 += p.chunk) {
        const int64_t nr = min(p.chunk, rows - r0);
        if (p.levels == 1) {
            hipLaunchKernelGGL((topk_tile_kernel<true, true>), dim3((unsigned)nr), dim3(kTopkThreads), 0, s, scores, ld, cols, seen_rowptr,
                               seen_col, nullptr, 0, 1, r0, k, p.kp, nullptr, 0, out_score, out_idx, out_count);
            continue;
        }
        hipLaunchKernelGGL((topk_tile_kernel<true, false>), dim3((unsigned)(p.tiles[0] * nr)), dim3(kTopkThreads), 0, s, scores, ld, cols,
                           seen_rowptr, seen_col, nullptr, 0, (int)p.tiles[0], r0, k, p.kp, bufA, p.n1, out_score, out_idx, out_count);
        unsigned long long* in = bufA;
        unsigned long long* out = bufB;
        int64_t n_in = p.n1;
        for (int L = 1; L < p.levels; ++L) {
            const int64_t t = p.tiles[L];
            if (L == p.levels - 1) {
                hipLaunchKernelGGL((topk_tile_kernel<false, true>), dim3((unsigned)(t * nr)), dim3(kTopkThreads), 0, s, scores, ld, cols,
                                   nullptr, nullptr, in, n_in, (int)t, r0, k, p.kp, nullptr, 0, out_score, out_idx, out_count);
            } else {
                const int64_t n_out = t * p.kp;
                hipLaunchKernelGGL((topk_tile_kernel<false, false>), dim3((unsigned)(t * nr)), dim3(kTopkThreads), 0, s, scores, ld, cols,
                                   nullptr, nullptr, in, n_in, (int)t, r0, k, p.kp, out, n_out, out_score, out_idx, out_count);
                unsigned long long* tmp = in;
                in = out;
                out = tmp;
                n_in = n_out;
            }
        }
    }
    return check_launch("ncf_topk_rows");
}
