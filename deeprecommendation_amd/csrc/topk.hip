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
// The levels above level 0 are also the merge levels of the fused score-and-select kernels (dot_topk.hip, mlp_topk.hip), whose
// first level writes kp keys per tile in the same layout: this file is the one owner of topk_tile_kernel and of the host side
// declared in topk_common.h (merge plan, workspace size, merge launches, the refusals every entry point shares).
#include "topk_common.h"

#include <utility>

namespace ncf {

struct TopkShared {
    uint32_t hist[kTopkThreads / kWave][256];
    unsigned long long sel[kTopkMaxK];
    uint32_t bitmap[kTopkTile / 32];
    unsigned long long red_min[kTopkThreads / kWave], red_max[kTopkThreads / kWave];
    int red_cnt[kTopkThreads / kWave];
    int bin, above, cnt_bin, nsel;
};

// LEVEL0: `src` is the score matrix (row-major, leading dimension ld); else the previous level's keys (n_in per row).
// FINAL: write sorted (score, column) pairs + counts; else write kp keys per tile into out_keys (n_out per row).
template <bool LEVEL0, bool FINAL>
__global__ __launch_bounds__(kTopkThreads) void topk_tile_kernel(
    const float* __restrict__ scores, int64_t ld, int64_t cols, const int64_t* __restrict__ seen_rowptr, const int32_t* __restrict__ seen_col,
    const unsigned long long* __restrict__ in_keys, int64_t n_in, int tiles, int64_t row0, int k, int kp,
    unsigned long long* __restrict__ out_keys, int64_t n_out, float* __restrict__ out_score, int32_t* __restrict__ out_idx,
    int32_t* __restrict__ out_count) {
    __shared__ TopkShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x % tiles;
    const int64_t rloc = blockIdx.x / tiles, row = row0 + rloc;
    const int64_t t0 = (int64_t)tile * kTopkTile;
    const int64_t n_total = LEVEL0 ? cols : n_in;
    const int n = (int)min((int64_t)kTopkTile, n_total - t0);

    unsigned long long key[kTopkPer];
    if (LEVEL0) {
        const bool excl = seen_rowptr != nullptr;
        if (excl) {
            sh.bitmap[tid] = 0u;
            __syncthreads();
            const int64_t b = seen_rowptr[row], e = seen_rowptr[row + 1];
            for (int64_t p = b + tid; p < e; p += kTopkThreads) {
                const int64_t c = (int64_t)seen_col[p] - t0;   // duplicates and ids outside [0, cols) fall out here or do nothing
                if (c >= 0 && c < n) atomicOr(&sh.bitmap[c >> 5], 1u << (c & 31));
            }
            __syncthreads();
        }
        const float* src = scores + row * ld + t0;
        const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;   // e is a multiple of 4: every quad is then aligned
#pragma unroll
        for (int it = 0; it < kTopkPer / 4; ++it) {
            const int e = it * (kTopkThreads * 4) + tid * 4;
            float v[4];
            if (vec && e + 3 < n) {
                const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + e));
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = e + j < n ? src[e + j] : 0.f;
            }
            const uint32_t bits = excl ? sh.bitmap[e >> 5] >> (e & 31) : 0u;   // e % 4 == 0: the 4 bits are in one word
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = e + j < n && !((bits >> j) & 1u);
                const uint32_t col = (uint32_t)(t0 + e + j);
                key[it * 4 + j] = ok ? ((unsigned long long)topk_map(v[j]) << 32) | (0xFFFFFFFFu - col) : 0ull;
            }
        }
    } else {
        const unsigned long long* src = in_keys + rloc * n_in + t0;       // n_in and t0 even: 16-byte aligned pairs
#pragma unroll
        for (int it = 0; it < kTopkPer / 2; ++it) {
            const int e = it * (kTopkThreads * 2) + tid * 2;
            if (e < n) {
                const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + e));
                key[it * 2] = ((unsigned long long)q[1] << 32) | q[0];
                key[it * 2 + 1] = ((unsigned long long)q[3] << 32) | q[2];
            } else {
                key[it * 2] = key[it * 2 + 1] = 0ull;
            }
        }
    }

    // ---- valid count, min / max of the valid keys
    unsigned long long kmin = ~0ull, kmax = 0ull;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < kTopkPer; ++i) {
        if (key[i]) {
            ++cnt;
            kmin = min(kmin, key[i]);
            kmax = max(kmax, key[i]);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        cnt += __shfl_xor(cnt, m);
        kmin = min(kmin, shfl_xor_u64(kmin, m));
        kmax = max(kmax, shfl_xor_u64(kmax, m));
    }
    if (lane == 0) {
        sh.red_cnt[wave] = cnt;
        sh.red_min[wave] = kmin;
        sh.red_max[wave] = kmax;
    }
    if (tid == 0) sh.nsel = 0;
    __syncthreads();
    cnt = 0;
    kmin = ~0ull;
    kmax = 0ull;
#pragma unroll
    for (int w = 0; w < kTopkThreads / kWave; ++w) {
        cnt += sh.red_cnt[w];
        kmin = min(kmin, sh.red_min[w]);
        kmax = max(kmax, sh.red_max[w]);
    }

    // ---- radix select: thr = the smallest key that is selected (every valid key >= thr is, and there are min(k, cnt) of them)
    unsigned long long thr = 1ull;
    if (cnt > k) {
        int top = 64 - __builtin_clzll(kmin ^ kmax);    // bits [top, 64) are common to every valid key (kmin != kmax: cnt > 1)
        unsigned long long prefix = kmax;
        int need = k;
        while (true) {
            const int shift = max(top - 8, 0);
            const uint32_t dmask = (1u << (top - shift)) - 1u;
#pragma unroll
            for (int i = tid; i < (kTopkThreads / kWave) * 256; i += kTopkThreads) (&sh.hist[0][0])[i] = 0u;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kTopkPer; ++i)
                if (key[i] && topk_high_eq(key[i], prefix, top)) atomicAdd(&sh.hist[wave][(uint32_t)(key[i] >> shift) & dmask], 1u);
            __syncthreads();
            if (wave == 0) {
                // lane l holds bins 255-4l .. 252-4l (descending); an inclusive scan over lanes finds the bin of the need-th key
                uint32_t c[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int b = 255 - 4 * lane - q;
                    c[q] = sh.hist[0][b] + sh.hist[1][b] + sh.hist[2][b] + sh.hist[3][b];
                    s += c[q];
                }
                uint32_t incl = s;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(incl, d);
                    if (lane >= d) incl += o;
                }
                const uint32_t excl = incl - s;
                if (excl < (uint32_t)need && (uint32_t)need <= incl) {
                    uint32_t run = excl;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (run < (uint32_t)need && (uint32_t)need <= run + c[q]) {
                            sh.bin = 255 - 4 * lane - q;
                            sh.above = (int)run;
                            sh.cnt_bin = (int)c[q];
                        }
                        run += c[q];
                    }
                }
            }
            __syncthreads();
            const int bin = sh.bin, above = sh.above, cnt_bin = sh.cnt_bin;
            __syncthreads();                            // every thread has read them before the next pass overwrites
            const unsigned long long lowmask = top >= 64 ? ~0ull : ((1ull << top) - 1ull);
            prefix = (prefix & ~lowmask) | ((unsigned long long)bin << shift);
            need -= above;
            top = shift;
            if (cnt_bin == need || top == 0) break;     // keys are unique: at top == 0 the bucket is one key
        }
        thr = top == 0 ? prefix : (prefix & ~((1ull << top) - 1ull));
    }

    // ---- gather the selected keys in LDS
#pragma unroll
    for (int i = 0; i < kTopkPer; ++i) {
        if (key[i] && key[i] >= thr) {
            const int p = atomicAdd(&sh.nsel, 1);
            if (p < kTopkMaxK) sh.sel[p] = key[i];
        }
    }
    __syncthreads();
    const int nsel = min(sh.nsel, k);

    if (!FINAL) {
        unsigned long long* dst = out_keys + rloc * n_out + (int64_t)tile * kp;
        for (int s = tid; s < kp; s += kTopkThreads) dst[s] = s < nsel ? sh.sel[s] : 0ull;
        return;
    }
    // ---- bitonic sort (descending) of the survivors, padded with 0 keys to a power of two
    int P = 2;
    while (P < nsel) P <<= 1;
    for (int s = nsel + tid; s < P; s += kTopkThreads) sh.sel[s] = 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += kTopkThreads) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = sh.sel[lo], b = sh.sel[hi];
                if ((a < b) == desc) {
                    sh.sel[lo] = b;
                    sh.sel[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const float* srow = scores ? scores + row * ld : nullptr;
    for (int s = tid; s < k; s += kTopkThreads) {
        if (s < nsel) {
            const uint32_t col = 0xFFFFFFFFu - (uint32_t)sh.sel[s];
            out_idx[row * k + s] = (int32_t)col;
            out_score[row * k + s] = scores ? srow[col] : topk_unmap((uint32_t)(sh.sel[s] >> 32));
        } else {
            out_idx[row * k + s] = -1;
            out_score[row * k + s] = -__builtin_inff();
        }
    }
    if (tid == 0) out_count[row] = nsel;
}

TopkMerge topk_merge_plan(int64_t rows, int64_t n1, int k, int64_t align) {
    TopkMerge p{};
    p.kp = topk_kp(k);
    p.n1 = n1;
    for (int64_t n = n1; n > 0;) {
        const int64_t t = (n + kTopkTile - 1) / kTopkTile;
        p.tiles[p.levels++] = t;
        n = t == 1 ? 0 : t * p.kp;
    }
    p.n2 = p.levels > 1 ? p.tiles[0] * p.kp : 0;
    const int64_t per_row = (p.n1 + p.n2) * 8;
    p.chunk = per_row ? max((int64_t)1, min(rows, (int64_t)(kTopkChunkBytes / per_row))) : rows;
    if (p.chunk < rows && p.chunk > align) p.chunk -= p.chunk % align;
    return p;
}

size_t topk_merge_bytes(const TopkMerge& p) { return (size_t)(p.chunk * (p.n1 + p.n2) * 8); }

void topk_merge(const TopkMerge& p, unsigned long long* bufA, const float* scores, int64_t ld, int64_t r0, int64_t nr, int k,
                float* out_score, int32_t* out_idx, int32_t* out_count, hipStream_t s) {
    unsigned long long* in = bufA;
    unsigned long long* out = bufA + p.chunk * p.n1;
    int64_t n_in = p.n1;
    for (int L = 0; L < p.levels; ++L) {
        const int64_t t = p.tiles[L];
        if (L == p.levels - 1) {
            hipLaunchKernelGGL((topk_tile_kernel<false, true>), dim3((unsigned)(t * nr)), dim3(kTopkThreads), 0, s, scores, ld, 0, nullptr,
                               nullptr, in, n_in, (int)t, r0, k, p.kp, nullptr, 0, out_score, out_idx, out_count);
        } else {
            const int64_t n_out = t * p.kp;
            hipLaunchKernelGGL((topk_tile_kernel<false, false>), dim3((unsigned)(t * nr)), dim3(kTopkThreads), 0, s, scores, ld, 0, nullptr,
                               nullptr, in, n_in, (int)t, r0, k, p.kp, out, n_out, out_score, out_idx, out_count);
            std::swap(in, out);
            n_in = n_out;
        }
    }
}

int topk_check_k(const char* what, int k, int fused_max_k) {
    if (k < 1 || k > kTopkMaxK) return fail(NCF_EINVAL, "%s: k = %d is outside 1 .. %d", what, k, kTopkMaxK);
    if (k > fused_max_k) return fail(NCF_EUNSUPPORTED, "%s: k = %d is above the fused limit %d", what, k, fused_max_k);
    return NCF_OK;
}

int topk_check_size(const char* what, int64_t rows, int64_t cols) {
    if (cols < 1 || cols > kTopkMaxCols)
        return fail(NCF_EUNSUPPORTED, "%s: cols = %lld is outside 1 .. %lld", what, (long long)cols, (long long)kTopkMaxCols);
    if (rows < 0 || rows > kTopkMaxRows)
        return fail(NCF_EUNSUPPORTED, "%s: rows = %lld is outside 0 .. %lld", what, (long long)rows, (long long)kTopkMaxRows);
    return NCF_OK;
}

int topk_check_buffers(const char* what, const char* query, const int64_t* seen_rowptr, const int32_t* seen_col, const void* workspace,
                       size_t workspace_bytes, size_t need) {
    if ((seen_rowptr == nullptr) != (seen_col == nullptr))
        return fail(NCF_EINVAL, "%s: seen_rowptr and seen_col are given together or not at all", what);
    if (workspace_bytes < need)
        return fail(NCF_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", what, workspace_bytes, need, query);
    if (need && (!workspace || !aligned16(workspace))) return fail(NCF_EINVAL, "%s: workspace must be 16-byte aligned", what);
    return NCF_OK;
}

// level 0 over the columns; a row longer than one tile leaves its tiles' keys to the merge levels
TopkMerge topk_rows_plan(int64_t rows, int64_t cols, int k) {
    const int64_t tiles0 = (cols + kTopkTile - 1) / kTopkTile;
    return topk_merge_plan(rows, tiles0 > 1 ? tiles0 * topk_kp(k) : 0, k);
}

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_topk_workspace_bytes(int64_t rows, int64_t cols, int k) {
    if (k < 1 || k > kTopkMaxK || cols < 1 || cols > kTopkMaxCols || rows < 1 || rows > kTopkMaxRows) return 0;   // no error string
    return topk_merge_bytes(topk_rows_plan(rows, cols, k));
}

extern "C" int ncf_topk_rows(const float* scores, int64_t rows, int64_t cols, int64_t ld, const int64_t* seen_rowptr, const int32_t* seen_col,
                             int k, float* out_score, int32_t* out_idx, int32_t* out_count, void* workspace, size_t workspace_bytes,
                             ncf_stream_t stream) {
    if (const int rc = topk_check_k("ncf_topk_rows", k, kTopkMaxK)) return rc;
    if (const int rc = topk_check_size("ncf_topk_rows", rows, cols)) return rc;
    if (ld < cols) return fail(NCF_EINVAL, "ncf_topk_rows: ld = %lld < cols = %lld", (long long)ld, (long long)cols);
    if (rows == 0) return NCF_OK;
    if (!scores || !out_score || !out_idx || !out_count) return fail(NCF_EINVAL, "ncf_topk_rows: null argument");
    const TopkMerge p = topk_rows_plan(rows, cols, k);
    if (const int rc = topk_check_buffers("ncf_topk_rows", "ncf_topk_workspace_bytes", seen_rowptr, seen_col, workspace, workspace_bytes,
                                          topk_merge_bytes(p)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    const int64_t tiles0 = (cols + kTopkTile - 1) / kTopkTile;
    for (int64_t r0 = 0; r0 < rows; r0 += p.chunk) {
        const int64_t nr = min(p.chunk, rows - r0);
        if (p.levels == 0) {
            hipLaunchKernelGGL((topk_tile_kernel<true, true>), dim3((unsigned)nr), dim3(kTopkThreads), 0, s, scores, ld, cols, seen_rowptr,
                               seen_col, nullptr, 0, 1, r0, k, p.kp, nullptr, 0, out_score, out_idx, out_count);
            continue;
        }
        hipLaunchKernelGGL((topk_tile_kernel<true, false>), dim3((unsigned)(tiles0 * nr)), dim3(kTopkThreads), 0, s, scores, ld, cols,
                           seen_rowptr, seen_col, nullptr, 0, (int)tiles0, r0, k, p.kp, keys, p.n1, out_score, out_idx, out_count);
        topk_merge(p, keys, scores, ld, r0, nr, k, out_score, out_idx, out_count, s);
    }
    return check_launch("ncf_topk_rows");
}
