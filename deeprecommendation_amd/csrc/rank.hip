// Exact full-catalogue ranks (ncf_rank_rows, ncf_dot_rank; ncf_mlp_rank lives beside its scoring code in mlp_topk.hip): where
// each held-out column of a row stands among all of the row's non-excluded columns, in the top-K kernels' key order — the
// quantity behind HR@K / NDCG@K / MRR / AUC.  Contract and the shared pieces: rank_common.h.
//
//   ncf_rank_rows   ranks the listed columns of an existing score matrix.  One 256-thread workgroup per (row, 8192-column tile)
//                   holds the tile's keys in registers (32 per thread, excluded columns as key 0 through an LDS bitmap, as
//                   topk_tile_kernel's level 0 does) and walks the row's target chunks of kRankMaxTargets entries: any number of
//                   targets per row, the scores read once.
//   ncf_dot_rank    never writes the score matrix: dot_topk_kernel's scoring half (dot_frag.h; the same MFMA chain layout and the
//                   same 15-add tree, so every score is gather_dot_kernel<false>'s bit for bit) with a counting sink instead of
//                   the candidate buffer.  The target's own score comes from ncf_gather_dot over the (row, target) pairs.
//                   ONE (max_targets == 1): each lane keeps its four users' target keys and counters in registers; the only LDS
//                   is the exclusion bitmap.  Else the users' sorted chunks and histograms live in dynamic LDS.
#include "dot_frag.h"
#include "rank_common.h"

namespace ncf {

constexpr int kRankThreads = 256;

// ---------------------------------------------------------------------------------------------------- preparation
// wave per row: the pair ids of the row's target entries
__global__ __launch_bounds__(kRankThreads) void rank_expand_kernel(const int64_t* __restrict__ user_ids, const int64_t* __restrict__ item_ids,
                                                                   int64_t rows, int64_t cols, const int64_t* __restrict__ tgt_rowptr,
                                                                   const int32_t* __restrict__ tgt_col, int64_t n_targets,
                                                                   int64_t* __restrict__ pair_user, int64_t* __restrict__ pair_item) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kRankThreads / kWave) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t u = user_ids ? user_ids[r] : r;
    const int64_t pb = max((int64_t)0, tgt_rowptr[r]), pe = min(n_targets, tgt_rowptr[r + 1]);
    for (int64_t e = pb + lane; e < pe; e += kWave) {
        const int64_t c = tgt_col[e];
        pair_user[e] = u;
        pair_item[e] = (c >= 0 && c < cols) ? (item_ids ? item_ids[c] : c) : 0;
    }
}

// workgroup per row: per chunk of `cap` entries the keys (kRankNoKey for a target outside [0, cols) or in the row's exclusion
// list), sorted ascending with their places; rank <- 0 / -1
__global__ __launch_bounds__(kRankThreads) void rank_prep_kernel(const float* __restrict__ scores, int64_t ld, const float* __restrict__ pair_score,
                                                                 int64_t cols, const int64_t* __restrict__ seen_rowptr,
                                                                 const int32_t* __restrict__ seen_col, const int64_t* __restrict__ tgt_rowptr,
                                                                 const int32_t* __restrict__ tgt_col, int cap, int single,
                                                                 unsigned long long* __restrict__ skey, int32_t* __restrict__ sperm,
                                                                 int32_t* __restrict__ rank, int32_t* overflow) {
    __shared__ unsigned long long s_key[kRankMaxTargets];
    __shared__ int s_idx[kRankMaxTargets], s_col[kRankMaxTargets], s_ok[kRankMaxTargets];
    __shared__ uint32_t s_filter[64];                     // which (column mod 2048) some target of the chunk has
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t pb = tgt_rowptr[row];
    int64_t pe = tgt_rowptr[row + 1];
    if (single && pe - pb > cap) {                        // more targets than the fused call was sized for: flagged, not ranked
        if (tid == 0 && overflow) *overflow = 1;
        for (int64_t e = pb + cap + tid; e < pe; e += kRankThreads) rank[e] = -1;
        pe = pb + cap;
    }
    for (int64_t base = pb; base < pe; base += cap) {
        const int n = (int)min((int64_t)cap, pe - base);
        int P = 2;
        while (P < n) P <<= 1;
        if (tid < 64) s_filter[tid] = 0u;
        __syncthreads();
        if (tid < n) {
            const int col = tgt_col[base + tid];
            const bool ok = col >= 0 && col < cols;
            s_col[tid] = col;
            s_ok[tid] = ok ? 1 : 0;
            if (ok) atomicOr(&s_filter[(col >> 5) & 63], 1u << (col & 31));
        }
        __syncthreads();
        if (seen_rowptr) {
            const int64_t sb = seen_rowptr[row], se = seen_rowptr[row + 1];
            for (int64_t p = sb + tid; p < se; p += kRankThreads) {
                const int c = seen_col[p];
                if (c < 0 || c >= cols || !((s_filter[(c >> 5) & 63] >> (c & 31)) & 1u)) continue;
                for (int t = 0; t < n; ++t)
                    if (s_col[t] == c) s_ok[t] = 0;
            }
            __syncthreads();
        }
        if (tid < P) {
            unsigned long long key = kRankNoKey;
            if (tid < n) {
                const bool ok = s_ok[tid] != 0;
                if (ok) key = rank_key(scores ? scores[row * ld + s_col[tid]] : pair_score[base + tid], s_col[tid]);
                rank[base + tid] = ok ? 0 : -1;
            }
            s_key[tid] = key;
            s_idx[tid] = tid;
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {      // bitonic, ascending by (key, place)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (tid < P / 2) {
                    const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
                    const bool asc = (lo & size) == 0;
                    const unsigned long long a = s_key[lo], b = s_key[hi];
                    const int ia = s_idx[lo], ib = s_idx[hi];
                    const bool gt = a > b || (a == b && ia > ib);
                    if (gt == asc) {
                        s_key[lo] = b; s_key[hi] = a;
                        s_idx[lo] = ib; s_idx[hi] = ia;
                    }
                }
                __syncthreads();
            }
        }
        if (tid < n) {
            skey[base + tid] = s_key[tid];
            sperm[base + tid] = s_idx[tid];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- ncf_rank_rows
__global__ __launch_bounds__(kRankThreads) void rank_rows_kernel(const float* __restrict__ scores, int64_t ld, int64_t cols,
                                                                 const int64_t* __restrict__ seen_rowptr, const int32_t* __restrict__ seen_col,
                                                                 const int64_t* __restrict__ tgt_rowptr, const unsigned long long* __restrict__ skey,
                                                                 const int32_t* __restrict__ sperm, int tiles, int32_t* __restrict__ rank,
                                                                 int32_t* __restrict__ ranked) {
    __shared__ unsigned long long s_key[kRankMaxTargets];
    __shared__ uint32_t s_hist[kRankMaxTargets + 1];
    __shared__ uint32_t s_bitmap[kTopkTile / 32];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const int64_t row = blockIdx.x / tiles;
    const int64_t t0 = (int64_t)tile * kTopkTile;
    const int n = (int)min((int64_t)kTopkTile, cols - t0);
    const bool excl = seen_rowptr != nullptr;
    if (excl) {
        s_bitmap[tid] = 0u;
        __syncthreads();
        const int64_t b = seen_rowptr[row], e = seen_rowptr[row + 1];
        for (int64_t p = b + tid; p < e; p += kRankThreads) {
            const int64_t c = (int64_t)seen_col[p] - t0;   // duplicates and ids outside [0, cols) fall out here or do nothing
            if (c >= 0 && c < n) atomicOr(&s_bitmap[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
    }
    unsigned long long key[kTopkPer];
    const float* src = scores + row * ld + t0;
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    int valid = 0;
#pragma unroll
    for (int it = 0; it < kTopkPer / 4; ++it) {
        const int e = it * (kRankThreads * 4) + tid * 4;
        float v[4];
        if (vec && e + 3 < n) {
            const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + e));
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = e + j < n ? src[e + j] : 0.f;
        }
        const uint32_t bits = excl ? s_bitmap[e >> 5] >> (e & 31) : 0u;   // e % 4 == 0: the 4 bits are in one word
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = e + j < n && !((bits >> j) & 1u);
            key[it * 4 + j] = ok ? rank_key(v[j], t0 + e + j) : 0ull;
            valid += ok ? 1 : 0;
        }
    }
    // ranked: one atomic per wave
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) valid += __shfl_xor(valid, m);
    if ((tid & 63) == 0 && valid) atomicAdd(&ranked[row], valid);

    const int64_t pb = tgt_rowptr[row], pe = tgt_rowptr[row + 1];
    for (int64_t base = pb; base < pe; base += kRankMaxTargets) {
        const int nt = (int)min((int64_t)kRankMaxTargets, pe - base);
        const int P = nt <= 2 ? 2 : 1 << (32 - __builtin_clz(nt - 1));
        __syncthreads();
        rank_stage(s_key, s_hist, skey + base, nt, P, tid, kRankThreads);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kTopkPer; ++i) {                  // fully unrolled: key[] stays in registers
            if (!key[i]) continue;
            const int p = rank_lower_bound(s_key, P, key[i]);
            if (p) atomicAdd(&s_hist[p], 1u);
        }
        __syncthreads();
        if (tid == 0) rank_suffix(s_hist, P);
        __syncthreads();
        rank_flush(s_key, s_hist, sperm + base, nt, rank + base, tid, kRankThreads);
    }
}

// ---------------------------------------------------------------------------------------------------- ncf_dot_rank
// dynamic LDS of one wave: [bitmap 16 x 64 words when there is an exclusion list][keys 16 x P][hist 16 x (P + 1)] (ONE: no keys / hist)
static size_t dot_rank_wave_bytes(bool excl, int max_targets) {
    size_t b = excl ? (size_t)kDtUsers * (kDtChunk / 32) * 4 : 0;
    if (max_targets > 1) {
        const int P = rank_slots(max_targets);
        b += (size_t)kDtUsers * P * 8 + (size_t)kDtUsers * (P + 1) * 4;
    }
    return b;
}

template <int J, bool ONE>
__global__ __launch_bounds__(kDtThreads) void dot_rank_kernel(
    const float* __restrict__ tabA, int64_t rowsA, int64_t ldA, const float* __restrict__ tabB, int64_t rowsB, int64_t ldB,
    const int64_t* __restrict__ idxA, const int64_t* __restrict__ idxB, int64_t cols, int D, const int64_t* __restrict__ seen_rowptr,
    const int32_t* __restrict__ seen_col, const int64_t* __restrict__ tgt_rowptr, const unsigned long long* __restrict__ skey,
    const int32_t* __restrict__ sperm, int64_t nrows, int tiles, int tile_cols, int max_targets, int P, int wave_bytes,
    int32_t* __restrict__ rank, int32_t* __restrict__ ranked, int32_t* oob) {
    extern __shared__ __attribute__((aligned(16))) char rank_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool excl = seen_rowptr != nullptr;
    char* wbase = rank_smem + (size_t)wave * wave_bytes;
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(wbase);                                    // [kDtUsers][kDtChunk / 32]
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(wbase + (excl ? kDtUsers * (kDtChunk / 32) * 4 : 0));  // [kDtUsers][P]
    uint32_t* hist = reinterpret_cast<uint32_t*>(keys + kDtUsers * P);                        // [kDtUsers][P + 1]
    const int tile = blockIdx.x % tiles;
    const int64_t u0 = (int64_t)(blockIdx.x / tiles) * kDtBlockUsers + wave * kDtUsers;       // first row of this wave
    if (u0 >= nrows) return;
    const int nu = (int)min((int64_t)kDtUsers, nrows - u0);
    const int r16 = lane & 15, q = lane >> 4;
    const bool vecA = (ldA & 3) == 0 && (reinterpret_cast<uintptr_t>(tabA) & 15u) == 0;
    const bool vecB = (ldB & 3) == 0 && (reinterpret_cast<uintptr_t>(tabB) & 15u) == 0;

    // this lane's user row (A operand: row r16)
    const float* arow = nullptr;
    if (r16 < nu) {
        const int64_t r = u0 + r16;
        const int64_t ia = idxA ? idxA[r] : r;
        if (ia >= 0 && ia < rowsA) arow = tabA + ia * ldA;
        else if (oob && q == 0) *oob = 1;
    }
    float a[J][16];
    load_frag<J>(arow, D, vecA, q, a);

    // the targets of the users whose scores this lane sees (C/D layout: users 4q .. 4q+3)
    unsigned long long tk[4];
    int cnt[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        tk[rr] = kRankNoKey;
        cnt[rr] = 0;
    }
    if (ONE) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int u = 4 * q + rr;
            if (u < nu) {
                const int64_t pb = tgt_rowptr[u0 + u];
                if (tgt_rowptr[u0 + u + 1] > pb) tk[rr] = skey[pb];
            }
        }
    } else {
        for (int u = 0; u < nu; ++u) {
            const int64_t pb = tgt_rowptr[u0 + u];
            const int n = (int)min((int64_t)max_targets, tgt_rowptr[u0 + u + 1] - pb);
            rank_stage(keys + u * P, hist + u * (P + 1), skey + pb, n, P, lane, kWave);
        }
        wave_lds_sync();
    }

    const int64_t c0 = (int64_t)tile * tile_cols, c1 = min(cols, c0 + tile_cols);
    const int steps = (int)((c1 - c0 + 15) >> 4);
    int excluded = 0;                                     // lane l: excluded columns of user l >> 2 in bitmap words 16 (l & 3) ..

    auto item_row = [&](int g) -> const float* {
        const int64_t c = c0 + (int64_t)g * 16 + r16;
        if (g >= steps || c >= c1) return nullptr;
        const int64_t ib = idxB ? idxB[c] : c;
        if (ib >= 0 && ib < rowsB) return tabB + ib * ldB;
        if (oob && q == 0) *oob = 1;
        return nullptr;
    };
    float b[J][16];
    load_frag<J>(item_row(0), D, vecB, q, b);

    for (int g = 0; g < steps; ++g) {
        const int64_t cbase = c0 + (int64_t)g * 16;
        if (excl && ((cbase - c0) % kDtChunk) == 0) {          // rebuild the exclusion bitmap for columns [cbase, cbase + kDtChunk)
            wave_lds_sync();
            for (int w = lane; w < kDtUsers * (kDtChunk / 32); w += kWave) bitmap[w] = 0u;
            wave_lds_sync();
            const int64_t span = min((int64_t)kDtChunk, c1 - cbase);
            for (int u = 0; u < nu; ++u) {
                const int64_t pb = seen_rowptr[u0 + u], pe = seen_rowptr[u0 + u + 1];
                for (int64_t p = pb + lane; p < pe; p += kWave) {
                    const int64_t c = (int64_t)seen_col[p] - cbase;     // ids outside the chunk (or the list) do nothing
                    if (c >= 0 && c < span) atomicOr(&bitmap[u * (kDtChunk / 32) + (c >> 5)], 1u << (c & 31));
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int i = 0; i < 16; ++i) excluded += __popc(bitmap[(lane >> 2) * (kDtChunk / 32) + (lane & 3) * 16 + i]);
        }
        float bn[J][16];
        load_frag<J>(item_row(g + 1), D, vecB, q, bn);        // next item block in flight during this one's MFMAs

        f32x4 acc[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int s = 0; s < 16; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][s], b[j][s], acc[s], 0, 0, 0);

        // lane holds item column r16 of users 4q .. 4q+3 (C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg)
        const int64_t c = cbase + r16;
        const uint32_t low = 0xFFFFFFFFu - (uint32_t)c;
        const int off = (int)((cbase - c0) % kDtChunk) + r16;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int u = 4 * q + rr;
            float p[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) p[s] = acc[s][rr];
            float qq[8], rs[4];
#pragma unroll
            for (int l = 0; l < 8; ++l) qq[l] = p[l] + p[l + 8];
#pragma unroll
            for (int l = 0; l < 4; ++l) rs[l] = qq[l] + qq[l + 4];
            const float score = (rs[0] + rs[2]) + (rs[1] + rs[3]);
            const unsigned long long key = ((unsigned long long)topk_map(score) << 32) | low;
            bool pass = u < nu && c < c1;
            if (excl) pass = pass && !((bitmap[u * (kDtChunk / 32) + (off >> 5)] >> (off & 31)) & 1u);
            if (ONE) {
                cnt[rr] += (pass && key > tk[rr]) ? 1 : 0;
            } else if (pass) {
                const int pos = rank_lower_bound(keys + u * P, P, key);
                if (pos) atomicAdd(&hist[u * (P + 1) + pos], 1u);
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int s = 0; s < 16; ++s) b[j][s] = bn[j][s];
    }

    // ---- this tile's counts into rank / ranked
    if (excl) {
        excluded += __shfl_xor(excluded, 1);
        excluded += __shfl_xor(excluded, 2);
        if ((lane & 3) == 0 && (lane >> 2) < nu) atomicAdd(&ranked[u0 + (lane >> 2)], (int)(c1 - c0) - excluded);
    } else if (lane < nu) {
        atomicAdd(&ranked[u0 + lane], (int)(c1 - c0));
    }
    if (ONE) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int v = cnt[rr];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            const int u = 4 * q + rr;
            if (r16 == 0 && u < nu && v && tk[rr] != kRankNoKey) atomicAdd(&rank[tgt_rowptr[u0 + u]], v);   // a chunk of one: place 0
        }
    } else {
        wave_lds_sync();
        if (lane < nu) rank_suffix(hist + lane * (P + 1), P);
        wave_lds_sync();
        for (int u = 0; u < nu; ++u) {
            const int64_t pb = tgt_rowptr[u0 + u];
            const int n = (int)min((int64_t)max_targets, tgt_rowptr[u0 + u + 1] - pb);
            rank_flush(keys + u * P, hist + u * (P + 1), sperm + pb, n, rank + pb, lane, kWave);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

size_t rank_ws_bytes(int64_t n_targets, bool fused) {
    const size_t n = (size_t)max((int64_t)1, n_targets);
    size_t b = up16(n * 8) + up16(n * 4);
    if (fused) b += 2 * up16(n * 8) + up16(n * 4);
    return b;
}

RankWs rank_ws_carve(void* workspace, int64_t n_targets, bool fused) {
    const size_t n = (size_t)max((int64_t)1, n_targets);
    char* p = (char*)workspace;
    RankWs w{};
    w.skey = (unsigned long long*)p; p += up16(n * 8);
    w.sperm = (int32_t*)p; p += up16(n * 4);
    if (fused) {
        w.pair_user = (int64_t*)p; p += up16(n * 8);
        w.pair_item = (int64_t*)p; p += up16(n * 8);
        w.pair_score = (float*)p;
    }
    return w;
}

int rank_check_max_targets(const char* what, int max_targets) {
    if (max_targets < 1) return fail(NCF_EINVAL, "%s: max_targets = %d is below 1", what, max_targets);
    if (max_targets > kRankMaxTargets)
        return fail(NCF_EUNSUPPORTED, "%s: max_targets = %d is above the fused limit %d", what, max_targets, kRankMaxTargets);
    return NCF_OK;
}

int rank_check_args(const char* what, const char* query, int64_t rows, const int64_t* seen_rowptr, const int32_t* seen_col,
                    const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, const int32_t* rank, const int32_t* ranked,
                    const void* workspace, size_t workspace_bytes, size_t need) {
    if (!tgt_rowptr || !tgt_col) return fail(NCF_EINVAL, "%s: the target CSR (rowptr, col) is required", what);
    if (!rank || !ranked) return fail(NCF_EINVAL, "%s: null output", what);
    return topk_check_buffers(what, query, seen_rowptr, seen_col, workspace, workspace_bytes, need);
}

void rank_expand(const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, const int64_t* tgt_rowptr,
                 const int32_t* tgt_col, int64_t n_targets, const RankWs& w, int32_t* ranked, hipStream_t s) {
    fill_u32_async(ranked, 0u, (size_t)rows * 4, s);
    if (n_targets <= 0) return;
    // entries of no listed row (a row subset) still go through the pair scorer: give them valid ids
    fill_u32_async(w.pair_user, 0u, (size_t)n_targets * 8, s);
    fill_u32_async(w.pair_item, 0u, (size_t)n_targets * 8, s);
    const int per = kRankThreads / kWave;
    hipLaunchKernelGGL(rank_expand_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(kRankThreads), 0, s, user_ids, item_ids, rows, cols,
                       tgt_rowptr, tgt_col, n_targets, w.pair_user, w.pair_item);
}

void rank_prepare(const float* scores, int64_t ld, const float* pair_score, int64_t rows, int64_t cols, const int64_t* seen_rowptr,
                  const int32_t* seen_col, const int64_t* tgt_rowptr, const int32_t* tgt_col, int cap, bool single, const RankWs& w,
                  int32_t* rank, int32_t* overflow, hipStream_t s) {
    hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)rows), dim3(kRankThreads), 0, s, scores, ld, pair_score, cols, seen_rowptr, seen_col,
                       tgt_rowptr, tgt_col, cap, single ? 1 : 0, w.skey, w.sperm, rank, overflow);
}

static int dot_rank_check(int64_t rows, int64_t cols, int D, int max_targets, const char* what) {
    if (const int rc = rank_check_max_targets(what, max_targets)) return rc;
    return dot_check_shape(what, rows, cols, D);
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_rank_max_targets(void) { return kRankMaxTargets; }

extern "C" size_t ncf_rank_rows_workspace_bytes(int64_t rows, int64_t cols, int64_t n_targets) {
    if (cols < 1 || cols > kTopkMaxCols || rows < 1 || rows > kTopkMaxRows || n_targets < 0) return 0;   // no error string
    return rank_ws_bytes(n_targets, false);
}

extern "C" int ncf_rank_rows(const float* scores, int64_t rows, int64_t cols, int64_t ld, const int64_t* seen_rowptr, const int32_t* seen_col,
                             const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, int32_t* rank, int32_t* ranked,
                             void* workspace, size_t workspace_bytes, ncf_stream_t stream) {
    if (const int rc = topk_check_size("ncf_rank_rows", rows, cols)) return rc;
    if (ld < cols) return fail(NCF_EINVAL, "ncf_rank_rows: ld = %lld < cols = %lld", (long long)ld, (long long)cols);
    if (n_targets < 0) return fail(NCF_EINVAL, "ncf_rank_rows: n_targets = %lld", (long long)n_targets);
    if (rows == 0) return NCF_OK;
    if (!scores) return fail(NCF_EINVAL, "ncf_rank_rows: null argument");
    if (const int rc = rank_check_args("ncf_rank_rows", "ncf_rank_rows_workspace_bytes", rows, seen_rowptr, seen_col, tgt_rowptr, tgt_col,
                                       n_targets, rank, ranked, workspace, workspace_bytes, rank_ws_bytes(n_targets, false)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const RankWs w = rank_ws_carve(workspace, n_targets, false);
    fill_u32_async(ranked, 0u, (size_t)rows * 4, s);
    rank_prepare(scores, ld, nullptr, rows, cols, seen_rowptr, seen_col, tgt_rowptr, tgt_col, kRankMaxTargets, false, w, rank, nullptr, s);
    const int64_t tiles = (cols + kTopkTile - 1) / kTopkTile;
    hipLaunchKernelGGL(rank_rows_kernel, dim3((unsigned)(rows * tiles)), dim3(kRankThreads), 0, s, scores, ld, cols, seen_rowptr, seen_col,
                       tgt_rowptr, w.skey, w.sperm, (int)tiles, rank, ranked);
    return check_launch("ncf_rank_rows");
}

extern "C" size_t ncf_dot_rank_workspace_bytes(int64_t rows, int64_t cols, int D, int64_t n_targets, int max_targets) {
    if (dot_rank_check(rows, cols, D, max_targets, "ncf_dot_rank_workspace_bytes") != NCF_OK || rows == 0 || n_targets < 0) return 0;
    return rank_ws_bytes(n_targets, true);
}

extern "C" int ncf_dot_rank(const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                            const int64_t* idxA, const int64_t* idxB, int64_t rows, int64_t cols, int D, const int64_t* seen_rowptr,
                            const int32_t* seen_col, const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, int max_targets,
                            int32_t* rank, int32_t* ranked, void* workspace, size_t workspace_bytes, int32_t* oob, int32_t* overflow,
                            ncf_stream_t stream) {
    if (const int rc = dot_rank_check(rows, cols, D, max_targets, "ncf_dot_rank")) return rc;
    if (n_targets < 0) return fail(NCF_EINVAL, "ncf_dot_rank: n_targets = %lld", (long long)n_targets);
    if (rows == 0) return NCF_OK;
    if (const int rc = dot_check_operands("ncf_dot_rank", tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, rows, cols, D, true)) return rc;
    if (const int rc = rank_check_args("ncf_dot_rank", "ncf_dot_rank_workspace_bytes", rows, seen_rowptr, seen_col, tgt_rowptr, tgt_col,
                                       n_targets, rank, ranked, workspace, workspace_bytes, rank_ws_bytes(n_targets, true)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const RankWs w = rank_ws_carve(workspace, n_targets, true);

    // the targets' own scores from the pair scorer, then their keys in order
    rank_expand(idxA, idxB, rows, cols, tgt_rowptr, tgt_col, n_targets, w, ranked, s);
    if (n_targets > 0) {
        if (const int rc = ncf_gather_dot(NCF_F32, tabA, rowsA, ldA, tabB, rowsB, ldB, w.pair_user, w.pair_item, n_targets, D, w.pair_score,
                                          oob, stream))
            return rc;
    }
    rank_prepare(nullptr, 0, w.pair_score, rows, cols, seen_rowptr, seen_col, tgt_rowptr, tgt_col, max_targets, true, w, rank, overflow, s);

    const int tile_cols = dot_topk_tile_cols(rows, cols);
    const int tiles = (int)((cols + tile_cols - 1) / tile_cols);
    const unsigned blocks = (unsigned)(((rows + kDtBlockUsers - 1) / kDtBlockUsers) * tiles);
    const bool one = max_targets == 1;
    const int P = rank_slots(max_targets);
    const int wave_bytes = (int)dot_rank_wave_bytes(seen_rowptr != nullptr, max_targets);
    const size_t lds = (size_t)wave_bytes * kDtWaves;
#define LAUNCH(J_, ONE_)                                                                                                                   \
    do {                                                                                                                                   \
        if (lds > 65536)                                                                                                                   \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dot_rank_kernel<J_, ONE_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);        \
        hipLaunchKernelGGL((dot_rank_kernel<J_, ONE_>), dim3(blocks), dim3(kDtThreads), lds, s, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, \
                           idxB, cols, D, seen_rowptr, seen_col, tgt_rowptr, w.skey, w.sperm, rows, tiles, tile_cols, max_targets, P,      \
                           wave_bytes, rank, ranked, oob);                                                                                 \
    } while (0)
#define LAUNCH_J(J_) do { if (one) LAUNCH(J_, true); else LAUNCH(J_, false); } while (0)
    NCF_DOT_DISPATCH(dot_steps(D), LAUNCH_J)
#undef LAUNCH_J
#undef LAUNCH
    return check_launch("ncf_dot_rank");
}

// ---------------------------------------------------------------------------------------------------- ncf_ranking_plan
// Host only.  Every figure comes from the function the entry point's launch calls (topk_rows_plan, dot_topk_tile_cols,
// dot_topk_plan, mlp_ranking_plan), after the entry point's own refusals on k / max_targets and on the size; the embedding width
// does not enter a plan, so its refusal is not made.
extern "C" int ncf_ranking_plan(int entry, int64_t rows, int64_t cols, int k_or_max_targets, int* tile_cols, int64_t* tiles,
                                int* merge_levels, int64_t* chunk_rows) {
    const char* what = "ncf_ranking_plan";
    int tc = kTopkTile;
    TopkMerge p{};
    bool merges = false;
    switch (entry) {
        case NCF_RANKING_TOPK_ROWS:
            if (const int rc = topk_check_k(what, k_or_max_targets, kTopkMaxK)) return rc;
            if (const int rc = topk_check_size(what, rows, cols)) return rc;
            p = topk_rows_plan(rows, cols, k_or_max_targets);
            merges = true;
            break;
        case NCF_RANKING_RANK_ROWS:
            if (const int rc = topk_check_size(what, rows, cols)) return rc;
            break;
        case NCF_RANKING_DOT_TOPK:
            if (const int rc = dot_topk_check_k(what, k_or_max_targets)) return rc;
            if (const int rc = topk_check_size(what, rows, cols)) return rc;
            tc = dot_topk_tile_cols(rows, cols);
            p = dot_topk_plan(rows, cols, tc, k_or_max_targets);
            merges = true;
            break;
        case NCF_RANKING_DOT_RANK:
            if (const int rc = rank_check_max_targets(what, k_or_max_targets)) return rc;
            if (const int rc = topk_check_size(what, rows, cols)) return rc;
            tc = dot_topk_tile_cols(rows, cols);
            break;
        case NCF_RANKING_MLP_TOPK:
            if (const int rc = mlp_ranking_plan(false, rows, cols, k_or_max_targets, what, &tc, &p)) return rc;
            merges = true;
            break;
        case NCF_RANKING_MLP_RANK:
            if (const int rc = mlp_ranking_plan(true, rows, cols, k_or_max_targets, what, &tc, &p)) return rc;
            break;
        default:
            return fail(NCF_EINVAL, "ncf_ranking_plan: entry = %d is not one of NCF_RANKING_*", entry);
    }
    if (tile_cols) *tile_cols = tc;
    if (tiles) *tiles = (cols + tc - 1) / tc;
    if (merge_levels) *merge_levels = merges ? p.levels : 0;
    if (chunk_rows) *chunk_rows = merges ? p.chunk : rows;
    return NCF_OK;
}
