// Full-catalogue softmax cross-entropy for a dot-product readout (ncf_dot_lse, ncf_dot_softmax_grad): the
// log-sum-exp of every listed row's logits over the whole catalogue, and the two gradients of the loss, without a B x N matrix.
// The scores are dot_topk.hip's (the chain layout and add tree documented there, the operand loads of dot_frag.h): bit-identical
// to gather_dot_kernel<false>.  A logit is z = score * tau, one rounded product.
//
// ncf_dot_lse: dot_topk_kernel's walk (4 independent waves, 16 rows each in registers, the other table's rows one block ahead)
// with a log-sum-exp sink: a lane keeps an online (m, l) for each of its 4 rows over its column residue, the 16 lanes of a row
// are merged by a fixed butterfly at the tile's end, and a second kernel merges the column tiles in ascending order.
//
// ncf_dot_softmax_grad: one kernel in two roles.  The RESIDENT side's 16 rows stay in registers, the WALKED side comes 16 rows
// at a time (rows = batch: resident batch rows walk the catalogue -> dA; rows = items: resident item rows walk the batch -> dQ).
// Per 16 x 16 block the score tile is made TRANSPOSED (walked rows as the MFMA's A operand, resident rows as B), so that its
// C registers (row 4q + reg = walked row, column = resident row) are already the B operand of
//     out^T (D x 16 resident) += walked^T (D x 16 walked) . w (16 walked x 16 resident),
// one K step of v_mfma_f32_16x16x4_f32 per reg (K slot q = walked row 4q + reg).  The walked rows' A operand is read from the
// wave's LDS copy of the block (the registers it was loaded into, stored with a chunk swizzle so that the four row groups of a
// read fall into four bank groups).  No float atomics: a split walk writes per-tile partial outputs that a second kernel adds in
// ascending tile order.
#include "dot_frag.h"

namespace ncf {

constexpr int64_t kDsMinTile = 64;                    // shortest walk tile
constexpr int64_t kDsTargetBlocks = 512;              // a walk is split until the grid reaches this
constexpr int64_t kDsPartialFloats = int64_t(8) << 20;   // partial outputs of one chunk of resident rows: 32 MiB

// The walk's tile: the whole walk rounded up to a power of two, halved (down to kDsMinTile) until resident blocks x tiles reaches
// kDsTargetBlocks.
inline int64_t ds_tile(int64_t resident, int64_t walk) {
    const int64_t rblocks = (resident + kDtBlockUsers - 1) / kDtBlockUsers;
    int64_t tile = kDsMinTile;
    while (tile < walk) tile <<= 1;
    while (tile > kDsMinTile && rblocks * ((walk + tile - 1) / tile) < kDsTargetBlocks) tile >>= 1;
    return tile;
}

struct DsPlan {
    int64_t tile, tiles;
    int64_t chunk;           // resident rows per launch (a multiple of kDtBlockUsers unless it is all of them)
};

// lse: every row in one launch (a partial is 8 bytes).  grad: a split walk keeps tiles x chunk x D partial floats <= kDsPartialFloats
inline DsPlan ds_plan(int64_t resident, int64_t walk, int D, bool grad) {
    DsPlan p;
    p.tile = ds_tile(resident, walk);
    p.tiles = (walk + p.tile - 1) / p.tile;
    p.chunk = resident;
    if (grad && p.tiles > 1) {
        const int64_t fit = kDsPartialFloats / (p.tiles * D) / kDtBlockUsers * kDtBlockUsers;
        p.chunk = min(resident, max((int64_t)kDtBlockUsers, fit));
    }
    return p;
}

inline size_t ds_lse_bytes(const DsPlan& p, int64_t rows) { return (size_t)p.tiles * rows * 2 * sizeof(float); }
inline size_t ds_grad_bytes(const DsPlan& p, int D) { return p.tiles > 1 ? (size_t)p.tiles * p.chunk * D * sizeof(float) : 0; }

// the 16 chain tiles of one block: rows = the rows of `ra` (the A operand), columns = the rows of `cb`
template <int J>
__device__ __forceinline__ void chain_tiles(const float (&ra)[J][16], const float (&cb)[J][16], f32x4 (&acc)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[j][s], cb[j][s], acc[s], 0, 0, 0);
}

// gather_dot_kernel<false>'s add tree over the 16 chains of C register rr
__device__ __forceinline__ float chain_tree(const f32x4 (&acc)[16], int rr) {
    float qq[8], rs[4];
#pragma unroll
    for (int l = 0; l < 8; ++l) qq[l] = acc[l][rr] + acc[l + 8][rr];
#pragma unroll
    for (int l = 0; l < 4; ++l) rs[l] = qq[l] + qq[l + 4];
    return (rs[0] + rs[2]) + (rs[1] + rs[3]);
}

// (m, l) <- the pair of the union; a side with m = -inf holds nothing
__device__ __forceinline__ void lse_merge(float& m, float& l, float m2, float l2) {
    const float M = fmaxf(m, m2);
    const float t1 = m == -INFINITY ? 0.f : __fmul_rn(l, expf(m - M));
    const float t2 = m2 == -INFINITY ? 0.f : __fmul_rn(l2, expf(m2 - M));
    m = M;
    l = t1 + t2;
}

template <int J>
__global__ __launch_bounds__(kDtThreads) void dot_lse_kernel(
    const float* __restrict__ tabA, int64_t rowsA, int64_t ldA, const float* __restrict__ tabB, int64_t rowsB, int64_t ldB,
    const int64_t* __restrict__ idxA, const int64_t* __restrict__ idxB, int64_t cols, int D, float tau, int64_t nrows, int tiles,
    int64_t tile_cols, float2* __restrict__ part, int32_t* oob) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x % tiles;
    const int64_t u0 = (int64_t)(blockIdx.x / tiles) * kDtBlockUsers + wave * kDtUsers;
    if (u0 >= nrows) return;
    const int nu = (int)min((int64_t)kDtUsers, nrows - u0);
    const int r16 = lane & 15, q = lane >> 4;
    const bool vecA = (ldA & 3) == 0 && (reinterpret_cast<uintptr_t>(tabA) & 15u) == 0;
    const bool vecB = (ldB & 3) == 0 && (reinterpret_cast<uintptr_t>(tabB) & 15u) == 0;

    const float* arow = nullptr;
    if (r16 < nu) {
        const int64_t r = u0 + r16;
        const int64_t ia = idxA ? idxA[r] : r;
        if (ia >= 0 && ia < rowsA) arow = tabA + ia * ldA;
        else if (oob && q == 0) *oob = 1;
    }
    float a[J][16];
    load_frag<J>(arow, D, vecA, q, a);

    const int64_t c0 = (int64_t)tile * tile_cols, c1 = min(cols, c0 + tile_cols);
    const int steps = (int)((c1 - c0 + 15) >> 4);
    auto item_row = [&](int g) -> const float* {
        const int64_t c = c0 + (int64_t)g * 16 + r16;
        if (g >= steps || c >= c1) return nullptr;
        const int64_t ib = idxB ? idxB[c] : c;
        if (ib >= 0 && ib < rowsB) return tabB + ib * ldB;
        if (oob && q == 0) *oob = 1;
        return nullptr;
    };
    const float* brow = item_row(0);
    float b[J][16];
    load_frag<J>(brow, D, vecB, q, b);

    float m[4], l[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) m[rr] = -INFINITY, l[rr] = 0.f;

    for (int g = 0; g < steps; ++g) {
        const float* bnext = item_row(g + 1);
        float bn[J][16];
        load_frag<J>(bnext, D, vecB, q, bn);
        f32x4 acc[16];
        chain_tiles<J>(a, b, acc);
        // lane holds column r16 of rows 4q .. 4q+3; a column outside the list or the table is in no denominator
        if (brow) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float z = __fmul_rn(chain_tree(acc, rr), tau);
                const float e = expf(-fabsf(z - m[rr]));          // m = -inf: 0
                if (z > m[rr]) {
                    l[rr] = __fmul_rn(l[rr], e) + 1.f;
                    m[rr] = z;
                } else {
                    l[rr] += e;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int s = 0; s < 16; ++s) b[j][s] = bn[j][s];
        brow = bnext;
    }

    // the 16 lanes of a row (one q group), by a fixed butterfly
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            const float m2 = __shfl_xor(m[rr], d), l2 = __shfl_xor(l[rr], d);
            lse_merge(m[rr], l[rr], m2, l2);
        }
        const int u = 4 * q + rr;
        if (r16 == 0 && u < nu) part[(int64_t)tile * nrows + u0 + u] = float2{m[rr], l[rr]};
    }
}

// the column tiles of a row in ascending order
__global__ void dot_lse_merge_kernel(const float2* __restrict__ part, int64_t rows, int tiles, float* __restrict__ lse, float* __restrict__ mx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float m = -INFINITY, l = 0.f;
    for (int t = 0; t < tiles; ++t) {
        const float2 p = part[(int64_t)t * rows + r];
        lse_merge(m, l, p.x, p.y);
    }
    lse[r] = m + logf(l);
    if (mx) mx[r] = m;
}

// ITEMS = false: resident = listed batch rows (tabR = the user table), walked = catalogue columns -> out row = dA of the batch row.
// ITEMS = true : resident = catalogue columns (tabR = the item table), walked = listed batch rows -> out row = dQ of the column.
// tgt / lse / gup are per batch row; `cols` is the catalogue's length (the range of a target).  out: row (tile * nr + local
// resident row), D floats: the result itself for tiles == 1, else the partials dot_grad_reduce_kernel adds.
template <int J, bool ITEMS>
__global__ __launch_bounds__(kDtThreads) void dot_softmax_grad_kernel(
    const float* __restrict__ tabR, int64_t rowsR, int64_t ldR, const int64_t* __restrict__ idxR, const float* __restrict__ tabW,
    int64_t rowsW, int64_t ldW, const int64_t* __restrict__ idxW, int64_t walk, int64_t cols, int D, float tau,
    const int64_t* __restrict__ tgt, const float* __restrict__ lse, const float* __restrict__ gup, int64_t r0, int64_t nr, int tiles,
    int64_t tile_len, float* __restrict__ out, int32_t* oob) {
    constexpr int S = 64 * J;                          // floats per staged row: 4 J chunks of 16
    __shared__ __attribute__((aligned(16))) float shw[kDtWaves][16 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sh = shw[wave];
    const int tile = blockIdx.x % tiles;
    const int64_t u0 = (int64_t)(blockIdx.x / tiles) * kDtBlockUsers + wave * kDtUsers;
    if (u0 >= nr) return;
    const int nu = (int)min((int64_t)kDtUsers, nr - u0);
    const int r16 = lane & 15, q = lane >> 4;
    const bool vecR = (ldR & 3) == 0 && (reinterpret_cast<uintptr_t>(tabR) & 15u) == 0;
    const bool vecW = (ldW & 3) == 0 && (reinterpret_cast<uintptr_t>(tabW) & 15u) == 0;

    // this lane's resident row (the score tile's column r16, the output's row)
    const int64_t rres = r0 + u0 + r16;
    const float* rrow = nullptr;
    bool rvalid = false;
    float r_lse = 0.f, r_gt = 0.f;
    int64_t r_t = -1;
    if (r16 < nu) {
        const int64_t ir = idxR ? idxR[rres] : rres;
        if (ir >= 0 && ir < rowsR) rrow = tabR + ir * ldR;
        else if (oob && q == 0) *oob = 1;
        rvalid = rrow != nullptr;
        if (!ITEMS) {
            r_t = tgt[rres];
            r_lse = lse[rres];
            if (r_t < 0 || r_t >= cols) {              // a target outside the catalogue: the row contributes zeros
                rvalid = false;
                if (oob && q == 0) *oob = 1;
            }
            r_gt = __fmul_rn(gup[rres], tau);
        }
    }
    float a[J][16];
    load_frag<J>(rrow, D, vecR, q, a);

    const int64_t w0 = (int64_t)tile * tile_len, w1 = min(walk, w0 + tile_len);
    const int steps = (int)((w1 - w0 + 15) >> 4);
    auto walked_row = [&](int g) -> const float* {
        const int64_t c = w0 + (int64_t)g * 16 + r16;
        if (g >= steps || c >= w1) return nullptr;
        const int64_t iw = idxW ? idxW[c] : c;
        if (iw >= 0 && iw < rowsW) return tabW + iw * ldW;
        if (oob && q == 0) *oob = 1;
        return nullptr;
    };
    const float* wrow = walked_row(0);
    float b[J][16];
    load_frag<J>(wrow, D, vecW, q, b);

    f32x4 o[4 * J];
#pragma unroll
    for (int dt = 0; dt < 4 * J; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int g = 0; g < steps; ++g) {
        const int64_t wbase = w0 + (int64_t)g * 16;
        const unsigned long long wmask = __ballot(wrow != nullptr);     // bit r (< 16): walked row r of this block is there
        const float* wnext = walked_row(g + 1);
        float bn[J][16];
        load_frag<J>(wnext, D, vecW, q, bn);

        // the walked block into LDS: row r16, chunk 4 j + q at the swizzled place (4 j + q) ^ ((r16 >> 2) & 3)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            float* dst = sh + r16 * S + 16 * ((kDtKS * j + q) ^ ((r16 >> 2) & 3));
#pragma unroll
            for (int h = 0; h < 4; ++h)
                *reinterpret_cast<f32x4*>(dst + 4 * h) = f32x4{b[j][4 * h], b[j][4 * h + 1], b[j][4 * h + 2], b[j][4 * h + 3]};
        }

        f32x4 acc[16];
        chain_tiles<J>(b, a, acc);                     // transposed: C row 4q + reg = walked row, column r16 = resident row

        // rows = items: lane r16 reads the walked batch row wbase + r16's (target, lse, g tau) once per block; a lane takes those
        // of its 4 rows by shuffle.  A target is < cols <= 2^24, so it travels as an int: -1 = no row, -2 = outside the catalogue
        int b_t = -1;
        float b_ls = 0.f, b_gt = 0.f;
        if (ITEMS && wbase + r16 < w1) {
            const int64_t t = tgt[wbase + r16];
            b_ls = lse[wbase + r16];
            b_gt = __fmul_rn(gup[wbase + r16], tau);
            b_t = (int)t;
            if (t < 0 || t >= cols) {
                b_t = -2;
                if (oob && q == 0) *oob = 1;
            }
        }

        float w[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int wr = 4 * q + reg;
            const float z = __fmul_rn(chain_tree(acc, reg), tau);
            bool ok = rvalid && ((wmask >> wr) & 1ull);
            float wv;
            if (!ITEMS) {
                const float p = expf(z - r_lse);
                wv = r_gt * (p - (wbase + wr == r_t ? 1.f : 0.f));
            } else {
                const int t = __shfl(b_t, wr);
                const float ls = __shfl(b_ls, wr), gt = __shfl(b_gt, wr);
                ok = ok && t != -2;
                const float p = expf(z - ls);
                wv = gt * (p - (rres == (int64_t)t ? 1.f : 0.f));
            }
            w[reg] = ok ? wv : 0.f;
        }

        wave_lds_sync();
#pragma unroll
        for (int dt = 0; dt < 4 * J; ++dt) {
            if (16 * dt < D) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const float av = sh[(4 * q + reg) * S + 16 * (dt ^ q) + r16];     // walked row 4q + reg, element 16 dt + r16
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[reg], o[dt], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int s = 0; s < 16; ++s) b[j][s] = bn[j][s];
        wrow = wnext;
    }

    // out^T tile dt: lane holds elements 16 dt + 4 q + i (i = 0 .. 3) of resident row r16
    if (r16 < nu) {
        float* dst = out + ((int64_t)tile * nr + u0 + r16) * D;
#pragma unroll
        for (int dt = 0; dt < 4 * J; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = 16 * dt + 4 * q + i;
                if (d < D) dst[d] = o[dt][i];
            }
    }
}

// out[e] = the partials of element e in ascending tile order
__global__ void dot_grad_reduce_kernel(const float* __restrict__ part, int64_t n, int tiles, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float acc = part[e];
    for (int t = 1; t < tiles; ++t) acc += part[(int64_t)t * n + e];
    out[e] = acc;
}

static int ds_check(const char* what, int64_t rows, int64_t cols, int D, float scale) {
    if (const int rc = dot_check_shape(what, rows, cols, D)) return rc;
    if (!(scale > 0.f) || !std::isfinite(scale)) return fail(NCF_EINVAL, "%s: scale = %g is not a finite number > 0", what, (double)scale);
    return NCF_OK;
}

static int ds_check_workspace(const char* what, const char* query, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace_bytes < need) return fail(NCF_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", what, workspace_bytes, need, query);
    if (need && (!workspace || !aligned16(workspace))) return fail(NCF_EINVAL, "%s: workspace must be 16-byte aligned", what);
    return NCF_OK;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_dot_softmax_plan(int kind, int64_t rows, int64_t cols, int D, int64_t* tile, int64_t* tiles, int64_t* chunk_rows) {
    const char* what = "ncf_dot_softmax_plan";
    if (kind < 0 || kind > 2) return fail(NCF_EINVAL, "%s: kind = %d is not one of NCF_DOT_SOFTMAX_*", what, kind);
    if (const int rc = dot_check_shape(what, rows, cols, D)) return rc;
    const bool items = kind == NCF_DOT_SOFTMAX_GRAD_ITEMS;
    const DsPlan p = ds_plan(items ? cols : rows, items ? rows : cols, D, kind != NCF_DOT_SOFTMAX_LSE);
    if (tile) *tile = p.tile;
    if (tiles) *tiles = p.tiles;
    if (chunk_rows) *chunk_rows = p.chunk;
    return NCF_OK;
}

extern "C" size_t ncf_dot_lse_workspace_bytes(int64_t rows, int64_t cols, int D) {
    if (dot_check_shape("ncf_dot_lse_workspace_bytes", rows, cols, D) != NCF_OK || rows == 0) return 0;
    return ds_lse_bytes(ds_plan(rows, cols, D, false), rows);
}

extern "C" int ncf_dot_lse(const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                           const int64_t* idxA, const int64_t* idxB, int64_t rows, int64_t cols, int D, float scale, float* out_lse,
                           float* out_max, void* workspace, size_t workspace_bytes, int32_t* oob, ncf_stream_t stream) {
    const char* what = "ncf_dot_lse";
    if (const int rc = ds_check(what, rows, cols, D, scale)) return rc;
    if (rows == 0) return NCF_OK;
    if (const int rc = dot_check_operands(what, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, rows, cols, D, out_lse != nullptr)) return rc;
    const DsPlan p = ds_plan(rows, cols, D, false);
    if (const int rc = ds_check_workspace(what, "ncf_dot_lse_workspace_bytes", workspace, workspace_bytes, ds_lse_bytes(p, rows))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float2* part = (float2*)workspace;
    const unsigned blocks = (unsigned)(((rows + kDtBlockUsers - 1) / kDtBlockUsers) * p.tiles);
#define LAUNCH(J_)                                                                                                                      \
    hipLaunchKernelGGL((dot_lse_kernel<J_>), dim3(blocks), dim3(kDtThreads), 0, s, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, cols, \
                       D, scale, rows, (int)p.tiles, p.tile, part, oob)
    NCF_DOT_DISPATCH(dot_steps(D), LAUNCH)
#undef LAUNCH
    hipLaunchKernelGGL(dot_lse_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, part, rows, (int)p.tiles, out_lse, out_max);
    return check_launch(what);
}

extern "C" size_t ncf_dot_softmax_grad_workspace_bytes(int64_t rows, int64_t cols, int D, int items) {
    if (dot_check_shape("ncf_dot_softmax_grad_workspace_bytes", rows, cols, D) != NCF_OK || rows == 0) return 0;
    return ds_grad_bytes(ds_plan(items ? cols : rows, items ? rows : cols, D, true), D);
}

extern "C" int ncf_dot_softmax_grad(const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                                    const int64_t* idxA, const int64_t* idxB, int64_t rows, int64_t cols, int D, const int64_t* targets,
                                    const float* lse, const float* g, float scale, int items, float* out, void* workspace,
                                    size_t workspace_bytes, int32_t* oob, ncf_stream_t stream) {
    const char* what = "ncf_dot_softmax_grad";
    if (const int rc = ds_check(what, rows, cols, D, scale)) return rc;
    if (rows == 0) return NCF_OK;
    if (const int rc = dot_check_operands(what, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA, idxB, rows, cols, D,
                                          targets && lse && g && out))
        return rc;
    const int64_t resident = items ? cols : rows, walk = items ? rows : cols;
    const DsPlan p = ds_plan(resident, walk, D, true);
    if (const int rc = ds_check_workspace(what, "ncf_dot_softmax_grad_workspace_bytes", workspace, workspace_bytes, ds_grad_bytes(p, D)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const float *tabR = items ? tabB : tabA, *tabW = items ? tabA : tabB;
    const int64_t rowsR = items ? rowsB : rowsA, ldR = items ? ldB : ldA, rowsW = items ? rowsA : rowsB, ldW = items ? ldA : ldB;
    const int64_t *idxR = items ? idxB : idxA, *idxW = items ? idxA : idxB;
    for (int64_t r0 = 0; r0 < resident; r0 += p.chunk) {
        const int64_t nr = min(p.chunk, resident - r0);
        float* final_rows = out + r0 * D;
        float* dst = p.tiles > 1 ? (float*)workspace : final_rows;
        const unsigned blocks = (unsigned)(((nr + kDtBlockUsers - 1) / kDtBlockUsers) * p.tiles);
#define LAUNCH_ROLE(J_, ITEMS_)                                                                                                        \
    hipLaunchKernelGGL((dot_softmax_grad_kernel<J_, ITEMS_>), dim3(blocks), dim3(kDtThreads), 0, s, tabR, rowsR, ldR, idxR, tabW, rowsW, \
                       ldW, idxW, walk, cols, D, scale, targets, lse, g, r0, nr, (int)p.tiles, p.tile, dst, oob)
#define LAUNCH(J_)                          \
    if (items) LAUNCH_ROLE(J_, true);       \
    else LAUNCH_ROLE(J_, false)
        NCF_DOT_DISPATCH(dot_steps(D), LAUNCH)
#undef LAUNCH
#undef LAUNCH_ROLE
        if (p.tiles > 1) {
            const int64_t n = nr * D;
            hipLaunchKernelGGL(dot_grad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)workspace, n,
                               (int)p.tiles, final_rows);
        }
    }
    return check_launch(what);
}
