// Fused dot-product score-and-select (ncf_dot_topk): the k best items of each listed user for a dot-product readout (MF,
// GraphNCF(use_dot_product=True)), without a B x I score matrix.  The scores are made in registers by f32 MFMA and filtered
// against a running per-user threshold before anything leaves the workgroup; only k keys per (user, column tile) are written.
//
// Scores: bit-identical to gather_dot_kernel<false> (gather.hip) for the same pair.  That kernel sums 16 fmaf chains (chain s
// over e = s, s+16, s+32, ... in increasing e, from +0.f) and adds them in a fixed tree (q_l = p_l + p_{l+8}, r_l = q_l + q_{l+4},
// t_l = r_l + r_{l+2}, score = t_0 + t_1).  Here each chain has its own 16 x 16 accumulator tile (16 users x 16 items) and
// v_mfma_f32_16x16x4_f32 advances it by kDtKS elements of the chain per step: K slot q of step j holds element 16 (kDtKS j + q) + s,
// so the K order inside one instruction is the chain's order (f32 MFMA is an exact fmaf chain over its K slots).  The 15 tree
// adds run on the VALU.
//
// Shape: a 256-thread workgroup owns 64 users (16 per wave) x one tile of tile_cols ranked-list columns.  The waves are
// independent (no workgroup barrier): each holds its 16 user rows in registers for the whole tile and walks the tile 16 items at
// a time (item rows read straight from global memory, one item-row block ahead; the four waves read the same rows, so three of
// four reads are L1 hits).  Per user the wave keeps kDtCap candidate keys in LDS and a threshold: a key is kept when it beats the
// threshold and its column is not excluded (an LDS bitmap of the user's excluded columns, rebuilt every kDtChunk columns).  A user
// whose buffer cannot take another 16 keys is re-selected down to k (wave-wide bitwise search for the k-th key, then
// compaction); the k-th key becomes the threshold.  At the end of the tile each user's k best keys go to the workspace in the
// layout topk_tile_kernel's merge levels read (kp keys per tile, 0-padded), and those levels (topk_merge, topk.hip) finish the
// ranking; the last one recovers the score from the key (topk_unmap), which is the caller's bits for every non-NaN score (a dot
// product from +0.f is never -0.0).
#include "dot_frag.h"

namespace ncf {

constexpr int kDtCap = 256;                        // candidate keys per user
constexpr int kDtMaxK = 128;                       // fused limit on k (a re-select must free >= 16 + some slots)

struct DtWaveShared {
    unsigned long long buf[kDtUsers][kDtCap];
    uint32_t bitmap[kDtUsers][kDtChunk / 32];
    unsigned long long thr[kDtUsers];
    int cnt[kDtUsers];
};

// keep the `keep` best of user u's candidates; the k-th becomes the threshold
__device__ void reselect(DtWaveShared& sh, int u, int keep, int lane) {
    const int n = sh.cnt[u];
    const unsigned long long kth = wave_reselect(sh.buf[u], n, keep, lane);
    if (lane == 0) {
        sh.cnt[u] = keep;
        sh.thr[u] = kth;
    }
    wave_lds_sync();
}

template <int J>
__global__ __launch_bounds__(kDtThreads) void dot_topk_kernel(
    const float* __restrict__ tabA, int64_t rowsA, int64_t ldA, const float* __restrict__ tabB, int64_t rowsB, int64_t ldB,
    const int64_t* __restrict__ idxA, const int64_t* __restrict__ idxB, int64_t cols, int D, const int64_t* __restrict__ seen_rowptr,
    const int32_t* __restrict__ seen_col, int64_t row0, int64_t nrows, int tiles, int tile_cols, int k, int kp,
    unsigned long long* __restrict__ out_keys, int64_t n_out, int32_t* oob) {
    __shared__ DtWaveShared shw[kDtWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    DtWaveShared& sh = shw[wave];
    const int tile = blockIdx.x % tiles;
    const int64_t u0 = (int64_t)(blockIdx.x / tiles) * kDtBlockUsers + wave * kDtUsers;   // first local row of this wave
    if (u0 >= nrows) return;
    const int nu = (int)min((int64_t)kDtUsers, nrows - u0);
    const int r16 = lane & 15, q = lane >> 4;
    const bool vecA = (ldA & 3) == 0 && (reinterpret_cast<uintptr_t>(tabA) & 15u) == 0;
    const bool vecB = (ldB & 3) == 0 && (reinterpret_cast<uintptr_t>(tabB) & 15u) == 0;

    // this lane's user row (A operand: row r16)
    const float* arow = nullptr;
    if (r16 < nu) {
        const int64_t r = row0 + u0 + r16;
        const int64_t ia = idxA ? idxA[r] : r;
        if (ia >= 0 && ia < rowsA) arow = tabA + ia * ldA;
        else if (oob && q == 0) *oob = 1;
    }
    float a[J][16];
    load_frag<J>(arow, D, vecA, q, a);

    if (lane < kDtUsers) {
        sh.cnt[lane] = 0;
        sh.thr[lane] = 0ull;
    }
    const int64_t c0 = (int64_t)tile * tile_cols, c1 = min(cols, c0 + tile_cols);
    const int steps = (int)((c1 - c0 + 15) >> 4);
    const bool excl = seen_rowptr != nullptr;

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
            for (int w = lane; w < kDtUsers * (kDtChunk / 32); w += kWave) (&sh.bitmap[0][0])[w] = 0u;
            wave_lds_sync();
            for (int u = 0; u < nu; ++u) {
                const int64_t r = row0 + u0 + u;
                const int64_t pb = seen_rowptr[r], pe = seen_rowptr[r + 1];
                for (int64_t p = pb + lane; p < pe; p += kWave) {
                    const int64_t c = (int64_t)seen_col[p] - cbase;     // ids outside the chunk (or the list) do nothing
                    if (c >= 0 && c < kDtChunk) atomicOr(&sh.bitmap[u][c >> 5], 1u << (c & 31));
                }
            }
            wave_lds_sync();
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
            bool pass = u < nu && c < c1 && key > sh.thr[u];
            if (pass && excl) {
                const int off = (int)((c - c0) % kDtChunk);
                pass = !((sh.bitmap[u][off >> 5] >> (off & 31)) & 1u);
            }
            if (pass) {
                const int slot = atomicAdd(&sh.cnt[u], 1);     // < kDtCap: a user had <= kDtCap - 16 before this step
                sh.buf[u][slot] = key;
            }
        }
        wave_lds_sync();
        unsigned long long full = __ballot(lane < kDtUsers && sh.cnt[lane] > kDtCap - 16);
        while (full) {
            const int u = __builtin_ctzll(full);
            full &= full - 1;
            reselect(sh, u, k, lane);
        }
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int s = 0; s < 16; ++s) b[j][s] = bn[j][s];
    }

    // each user's k best keys of this tile, unsorted, 0-padded to kp
    for (int u = 0; u < nu; ++u) {
        if (sh.cnt[u] > k) reselect(sh, u, k, lane);
        const int n = sh.cnt[u];
        unsigned long long* dst = out_keys + (u0 + u) * n_out + (int64_t)tile * kp;
        for (int s = lane; s < kp; s += kWave) dst[s] = s < n ? sh.buf[u][s] : 0ull;
    }
}

// the merge levels after it, over kp keys per tile, in chunks of whole user blocks
TopkMerge dot_topk_plan(int64_t rows, int64_t cols, int tile_cols, int k) {
    return topk_merge_plan(rows, (cols + tile_cols - 1) / tile_cols * topk_kp(k), k, kDtBlockUsers);
}

int dot_topk_check_k(const char* what, int k) { return topk_check_k(what, k, kDtMaxK); }

static int dot_topk_check(int64_t rows, int64_t cols, int D, int k, const char* what) {
    if (const int rc = dot_topk_check_k(what, k)) return rc;
    return dot_check_shape(what, rows, cols, D);
}

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_dot_topk_workspace_bytes(int64_t rows, int64_t cols, int D, int k) {
    if (dot_topk_check(rows, cols, D, k, "ncf_dot_topk_workspace_bytes") != NCF_OK || rows == 0) return 0;
    return topk_merge_bytes(dot_topk_plan(rows, cols, dot_topk_tile_cols(rows, cols), k));
}

extern "C" int ncf_dot_topk(const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                            const int64_t* idxA, const int64_t* idxB, int64_t rows, int64_t cols, int D, const int64_t* seen_rowptr,
                            const int32_t* seen_col, int k, float* out_score, int32_t* out_idx, int32_t* out_count, void* workspace,
                            size_t workspace_bytes, int32_t* oob, ncf_stream_t stream) {
    if (const int rc = dot_topk_check(rows, cols, D, k, "ncf_dot_topk")) return rc;
    if (rows == 0) return NCF_OK;
    if (const int rc = dot_check_operands("ncf_dot_topk", tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, rows, cols, D,
                                          out_score && out_idx && out_count))
        return rc;
    const int tile_cols = dot_topk_tile_cols(rows, cols);
    const int tiles0 = (int)((cols + tile_cols - 1) / tile_cols);
    const TopkMerge p = dot_topk_plan(rows, cols, tile_cols, k);
    if (const int rc = topk_check_buffers("ncf_dot_topk", "ncf_dot_topk_workspace_bytes", seen_rowptr, seen_col, workspace, workspace_bytes,
                                          topk_merge_bytes(p)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    for (int64_t r0 = 0; r0 < rows; r0 += p.chunk) {
        const int64_t nr = min(p.chunk, rows - r0);
        const unsigned blocks = (unsigned)(((nr + kDtBlockUsers - 1) / kDtBlockUsers) * tiles0);
#define LAUNCH(J_)                                                                                                                       \
    hipLaunchKernelGGL((dot_topk_kernel<J_>), dim3(blocks), dim3(kDtThreads), 0, s, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, cols, \
                       D, seen_rowptr, seen_col, r0, nr, tiles0, tile_cols, k, p.kp, keys, p.n1, oob)
        NCF_DOT_DISPATCH(dot_steps(D), LAUNCH)
#undef LAUNCH
        // merge levels over the fused level's kp keys per tile; the last one sorts and writes (score from the key)
        topk_merge(p, keys, nullptr, 0, r0, nr, k, out_score, out_idx, out_count, s);
    }
    return check_launch("ncf_dot_topk");
}
