// ItemKNN, the neighbourhood collaborative-filtering baseline (Sarwar et al. 2001; Surprise KNNBasic, LensKit ItemItem) on gfx950:
// shrunk cosine similarities of the items over the rating matrix, a table of each item's N nearest neighbours, and scores
//     r^(u, i) = sum over the neighbours j of i that u rated of s_ij * v_uj   ( / sum of those s_ij ).
//
// The similarities are a sparse Gram matrix X^T X of the (U, I) rating matrix X.  ncf_knn_sim_rows computes rows of it WITHOUT float
// atomics and in a fixed summation order: one workgroup of ONE wave owns one (item i, tile of columns); the tile's dot / co-rating
// accumulators live in LDS; the wave walks the users of column i in ascending order (the transposed CSR), and for each user its lanes
// stride over the user's row (the user CSR) and add v_ui * v_uj into accumulator j.  A user holds an item at most once, so the lanes
// of one user never meet; a workgroup barrier between two users orders one user's LDS writes before the next user's reads.  The
// chain over the users of the most popular item is the floor of a fit, as the chain of a block is KernelMF's.
//
// Every id is checked before it is used as an address: a row, a column or a pointer outside its array sets the sticky out-of-range
// flag and that entry adds nothing; a row of the user CSR whose columns do not strictly ascend sets the entry's own sticky flag.
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py EXTRA_FLAGS): every product, sum, quotient and square root of the contract
// (include/ncf_abi.h) is rounded on its own.  The pragma below says the same to a build that forgets the flag.  hipcc's default fp32
// division and square root are correctly rounded and are relied on; no fast-math flag may be added to this file.
#include "ncf_common.h"
#include "gram_walk.h"

#include <math.h>

#pragma clang fp contract(off)

#define NCF_KNN_MAX_N 256
#define NCF_KNN_DEFAULT_TILE 2048         // columns per tile: 8 bytes of LDS each (16 KiB per one-wave workgroup)
#define NCF_KNN_MAX_TILE 8192             // 64 KiB
#define NCF_KNN_DEFAULT_STAGE 2048        // entries of a user's row staged in LDS by ncf_knn_scores (8 bytes each)
#define NCF_KNN_MAX_STAGE 8192
#define NCF_KNN_SCORE_THREADS 256

namespace ncf {

// sq[i] of the contract: one wave per item
__global__ __launch_bounds__(64) void knn_item_sq_kernel(const int64_t* __restrict__ colptr, const float* __restrict__ tval, int64_t nnz,
                                                         int64_t I, float* __restrict__ sq, int32_t* oob) {
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < I; i += gridDim.x) {
        int64_t beg, end;
        csr_range(colptr, i, nnz, lane == 0 ? oob : nullptr, beg, end);
        beg = uniform64(beg);
        end = uniform64(end);
        float part = 0.0f;
        for (int64_t e = beg + lane; e < end; e += 64) {
            const float v = tval[e];
            const float t = v * v;
            part = part + t;
        }
        part = part + __shfl_xor(part, 1);
        part = part + __shfl_xor(part, 2);
        part = part + __shfl_xor(part, 4);
        part = part + __shfl_xor(part, 8);
        part = part + __shfl_xor(part, 16);
        part = part + __shfl_xor(part, 32);
        if (lane == 0) sq[i] = part;
    }
}

// One (item, column tile) per one-wave workgroup: blockIdx.x = tile, blockIdx.y = item - i0.
__global__ __launch_bounds__(64) void knn_sim_rows_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t U,
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ row, const float* __restrict__ tval, int64_t nnzT, int64_t I,
    const float* __restrict__ sq, int64_t i0, int min_support, float shrink, int T, float* __restrict__ out, int64_t ldo, int32_t* oob,
    int32_t* order) {
    extern __shared__ __align__(16) unsigned char knn_lds[];
    float* dot = reinterpret_cast<float*>(knn_lds);
    int* co = reinterpret_cast<int*>(knn_lds) + T;
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int64_t i = i0 + blockIdx.y;
    const int64_t t0 = (int64_t)tile * T;
    const int64_t t1 = t0 + T < I ? t0 + T : I;
    const int tl = (int)(t1 - t0);
    gram_row_walk<true>(rowptr, col, val, nnz, U, colptr, row, tval, nnzT, I, i, tile, t0, t1, dot, co, oob, order);   // gram_walk.h
    const float sqi = sq[i];
    const float ri = sqrtf(sqi);
    float* orow = out + (int64_t)blockIdx.y * ldo;
    for (int j = lane; j < tl; j += 64) {
        const int64_t jj = t0 + j;
        const int c = co[j];
        const float rj = sqrtf(sq[jj]);
        const float n = ri * rj;
        float s = 0.0f;
        if (jj != i && c >= min_support && n != 0.0f) {
            const float cs = dot[j] / n;
            const float cf = (float)c;
            const float den = cf + shrink;
            const float sh = cf / den;
            const float v = cs * sh;
            if (v > 0.0f) s = v;
        }
        orow[jj] = s;
    }
}

// The score rule of the contract for one (user row, item): cols / vals are the row's n entries, in LDS or in global memory.
__device__ __forceinline__ float knn_score_one(const int32_t* cols, const float* vals, int n, const int32_t* __restrict__ nb_pos,
                                               const float* __restrict__ nb_sim, const int32_t* __restrict__ nb_cnt, int64_t I, int N,
                                               int64_t i, int weighted, float fill, int32_t* oob) {
    float num = 0.0f, den = 0.0f;
    int cnt = nb_cnt[i];
    cnt = cnt < 0 ? 0 : cnt > N ? N : cnt;
    const int32_t* pos = nb_pos + i * N;
    const float* sim = nb_sim + i * N;
    for (int t = 0; t < cnt; ++t) {
        const int j = pos[t];
        if (j < 0 || (int64_t)j >= I) {                    // -1 is the table's padding; anything else outside the items is flagged
            if (j != -1 && oob) atomicOr(oob, 1);
            continue;
        }
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cols[mid] < j) lo = mid + 1; else hi = mid;
        }
        if (lo < n && cols[lo] == j) {
            const float s = sim[t];
            const float sv = s * vals[lo];
            num = num + sv;
            den = den + s;
        }
    }
    if (!weighted) return num;
    return den > 0.0f ? num / den : fill;
}

// One workgroup per (user, tile of 256 items): blockIdx.x = tile, blockIdx.y = user of the list.
__global__ __launch_bounds__(NCF_KNN_SCORE_THREADS) void knn_scores_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t R,
    const int64_t* __restrict__ users, const int32_t* __restrict__ nb_pos, const float* __restrict__ nb_sim,
    const int32_t* __restrict__ nb_cnt, int64_t I, int N, int64_t i0, int64_t i1, int weighted, float fill, int stage_cap,
    float* __restrict__ out, int64_t ldo, int32_t* oob) {
    extern __shared__ __align__(16) unsigned char knn_lds[];
    int32_t* scol = reinterpret_cast<int32_t*>(knn_lds);
    float* sval = reinterpret_cast<float*>(knn_lds) + stage_cap;
    const int64_t b = blockIdx.y;
    const int64_t u = users[b];
    int64_t rb = 0, re = 0;
    if (u < 0 || u >= R) {                                 // nothing is read through this row: it scores as an empty one
        if (oob && threadIdx.x == 0) atomicOr(oob, 1);
    } else {
        csr_range(rowptr, u, nnz, threadIdx.x == 0 ? oob : nullptr, rb, re);
    }
    if (re - rb > 0x7fffffff) re = rb + 0x7fffffff;
    const int n = (int)(re - rb);
    const bool staged = n <= stage_cap;                    // uniform over the workgroup
    if (staged) {
        for (int e = threadIdx.x; e < n; e += NCF_KNN_SCORE_THREADS) {
            scol[e] = col[rb + e];
            sval[e] = val[rb + e];
        }
        __syncthreads();
    }
    const int64_t i = i0 + (int64_t)blockIdx.x * NCF_KNN_SCORE_THREADS + threadIdx.x;
    if (i >= i1) return;
    float r;
    if (staged)
        r = knn_score_one(scol, sval, n, nb_pos, nb_sim, nb_cnt, I, N, i, weighted, fill, oob);
    else
        r = knn_score_one(col + rb, val + rb, n, nb_pos, nb_sim, nb_cnt, I, N, i, weighted, fill, oob);
    out[b * ldo + (i - i0)] = r;
}

// One lane per (user row, item) pair.
__global__ __launch_bounds__(256) void knn_predict_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t R,
    const int64_t* __restrict__ users, const int64_t* __restrict__ items, int64_t n_pairs, const int32_t* __restrict__ nb_pos,
    const float* __restrict__ nb_sim, const int32_t* __restrict__ nb_cnt, int64_t I, int N, int weighted, float fill,
    float* __restrict__ out, int32_t* oob) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pairs) return;
    const int64_t u = users[k], i = items[k];
    float r = weighted ? fill : 0.0f;                      // what an empty row scores
    if (u < 0 || u >= R || i < 0 || i >= I) {
        if (oob) atomicOr(oob, 1);
    } else {
        int64_t rb, re;
        csr_range(rowptr, u, nnz, oob, rb, re);
        if (re - rb > 0x7fffffff) re = rb + 0x7fffffff;
        r = knn_score_one(col + rb, val + rb, (int)(re - rb), nb_pos, nb_sim, nb_cnt, I, N, i, weighted, fill, oob);
    }
    out[k] = r;
}

static int knn_check_table(const char* who, int64_t I, int N, int weighted, float fill) {
    if (I < 0) return fail(NCF_EINVAL, "%s: negative size I=%lld", who, (long long)I);
    if (N < 1 || N > NCF_KNN_MAX_N) return fail(NCF_EINVAL, "%s: N = %d neighbours per item (1 .. %d)", who, N, NCF_KNN_MAX_N);
    if (weighted != 0 && weighted != 1) return fail(NCF_EINVAL, "%s: weighted_average = %d (0 or 1)", who, weighted);
    if (!isfinite(fill)) return fail(NCF_EINVAL, "%s: fill is not finite", who);
    return NCF_OK;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_knn_item_sq(const int64_t* colptr, const float* tval, int64_t nnz, int64_t I, float* sq, int32_t* dev_oob_flag,
                               ncf_stream_t stream) {
    if (I < 0 || nnz < 0) return fail(NCF_EINVAL, "ncf_knn_item_sq: negative size I=%lld nnz=%lld", (long long)I, (long long)nnz);
    if (I > 0 && (!colptr || !sq)) return fail(NCF_EINVAL, "ncf_knn_item_sq: null column pointers or output");
    if (nnz > 0 && !tval) return fail(NCF_EINVAL, "ncf_knn_item_sq: %lld entries without values", (long long)nnz);
    if (I == 0) return NCF_OK;
    const unsigned blocks = (unsigned)(I < (1 << 20) ? I : (1 << 20));     // grid-stride beyond
    hipLaunchKernelGGL(knn_item_sq_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, colptr, tval, nnz, I, sq, dev_oob_flag);
    return check_launch("ncf_knn_item_sq");
}

extern "C" int ncf_knn_sim_rows(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t U, const int64_t* colptr,
                                const int32_t* row, const float* tval, int64_t nnzT, int64_t I, const float* sq, int64_t i0, int64_t i1,
                                int min_support, float shrink, int col_tile, float* out, int64_t ldo, int32_t* dev_oob_flag,
                                int32_t* dev_order_flag, ncf_stream_t stream) {
    const char* who = "ncf_knn_sim_rows";
    if (U < 0 || I < 0 || nnz < 0 || nnzT < 0)
        return fail(NCF_EINVAL, "%s: negative size U=%lld I=%lld nnz=%lld nnzT=%lld", who, (long long)U, (long long)I, (long long)nnz, (long long)nnzT);
    if (i0 < 0 || i1 < i0 || i1 > I) return fail(NCF_EINVAL, "%s: items [%lld, %lld) outside [0, %lld)", who, (long long)i0, (long long)i1, (long long)I);
    if (min_support < 1) return fail(NCF_EINVAL, "%s: min_support = %d", who, min_support);
    if (!isfinite(shrink) || shrink < 0.f) return fail(NCF_EINVAL, "%s: shrink must be finite and >= 0", who);
    if (col_tile < 0 || col_tile % 64 != 0 || col_tile > NCF_KNN_MAX_TILE)
        return fail(NCF_EINVAL, "%s: col_tile = %d (0, or a multiple of 64 up to %d)", who, col_tile, NCF_KNN_MAX_TILE);
    if (ldo < I) return fail(NCF_EINVAL, "%s: ldo = %lld < I = %lld", who, (long long)ldo, (long long)I);
    if (i1 - i0 > 65535) return fail(NCF_EUNSUPPORTED, "%s: %lld items in one call (at most 65535)", who, (long long)(i1 - i0));
    if (i1 > i0 && (!rowptr || !colptr || !sq || !out)) return fail(NCF_EINVAL, "%s: null pointers, norms or output", who);
    if (nnz > 0 && (!col || !val)) return fail(NCF_EINVAL, "%s: %lld entries without col / val", who, (long long)nnz);
    if (nnzT > 0 && (!row || !tval)) return fail(NCF_EINVAL, "%s: %lld transposed entries without row / tval", who, (long long)nnzT);
    if (i1 == i0) return NCF_OK;
    int T = col_tile;
    if (T == 0) {
        const int64_t up = (I + 63) / 64 * 64;
        T = (int)(up < NCF_KNN_DEFAULT_TILE ? up : NCF_KNN_DEFAULT_TILE);
    }
    const int64_t tiles = (I + T - 1) / T;
    if (tiles > 0x7fffffff) return fail(NCF_EUNSUPPORTED, "%s: %lld column tiles", who, (long long)tiles);
    hipLaunchKernelGGL(knn_sim_rows_kernel, dim3((unsigned)tiles, (unsigned)(i1 - i0)), dim3(64), (size_t)T * 8, (hipStream_t)stream, rowptr,
                       col, val, nnz, U, colptr, row, tval, nnzT, I, sq, i0, min_support, shrink, T, out, ldo, dev_oob_flag, dev_order_flag);
    return check_launch(who);
}

extern "C" int ncf_knn_scores(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t R, const int64_t* users,
                              int64_t B, const int32_t* nb_pos, const float* nb_sim, const int32_t* nb_cnt, int64_t I, int N, int64_t i0,
                              int64_t i1, int weighted_average, float fill, int stage_cap, float* out, int64_t ldo, int32_t* dev_oob_flag,
                              ncf_stream_t stream) {
    const char* who = "ncf_knn_scores";
    if (R < 0 || B < 0 || nnz < 0) return fail(NCF_EINVAL, "%s: negative size R=%lld B=%lld nnz=%lld", who, (long long)R, (long long)B, (long long)nnz);
    if (const int rc = knn_check_table(who, I, N, weighted_average, fill)) return rc;
    if (i0 < 0 || i1 < i0 || i1 > I) return fail(NCF_EINVAL, "%s: items [%lld, %lld) outside [0, %lld)", who, (long long)i0, (long long)i1, (long long)I);
    if (stage_cap < 0 || stage_cap > NCF_KNN_MAX_STAGE) return fail(NCF_EINVAL, "%s: stage_cap = %d (0 .. %d)", who, stage_cap, NCF_KNN_MAX_STAGE);
    if (ldo < i1 - i0) return fail(NCF_EINVAL, "%s: ldo = %lld < %lld items", who, (long long)ldo, (long long)(i1 - i0));
    if (B > 65535) return fail(NCF_EUNSUPPORTED, "%s: %lld users in one call (at most 65535)", who, (long long)B);
    const bool work = B > 0 && i1 > i0;
    if (work && (!rowptr || !users || !nb_pos || !nb_sim || !nb_cnt || !out)) return fail(NCF_EINVAL, "%s: null pointers, user list, table or output", who);
    if (work && nnz > 0 && (!col || !val)) return fail(NCF_EINVAL, "%s: %lld entries without col / val", who, (long long)nnz);
    if (!work) return NCF_OK;
    const int cap = stage_cap ? stage_cap : NCF_KNN_DEFAULT_STAGE;
    const int64_t tiles = (i1 - i0 + NCF_KNN_SCORE_THREADS - 1) / NCF_KNN_SCORE_THREADS;
    hipLaunchKernelGGL(knn_scores_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(NCF_KNN_SCORE_THREADS), (size_t)cap * 8, (hipStream_t)stream,
                       rowptr, col, val, nnz, R, users, nb_pos, nb_sim, nb_cnt, I, N, i0, i1, weighted_average, fill, cap, out, ldo, dev_oob_flag);
    return check_launch(who);
}

extern "C" int ncf_knn_predict(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t R, const int64_t* users,
                               const int64_t* items, int64_t n, const int32_t* nb_pos, const float* nb_sim, const int32_t* nb_cnt, int64_t I,
                               int N, int weighted_average, float fill, float* out, int32_t* dev_oob_flag, ncf_stream_t stream) {
    const char* who = "ncf_knn_predict";
    if (R < 0 || n < 0 || nnz < 0) return fail(NCF_EINVAL, "%s: negative size R=%lld n=%lld nnz=%lld", who, (long long)R, (long long)n, (long long)nnz);
    if (const int rc = knn_check_table(who, I, N, weighted_average, fill)) return rc;
    if (n > 0 && (!rowptr || !users || !items || !nb_pos || !nb_sim || !nb_cnt || !out))
        return fail(NCF_EINVAL, "%s: null pointers, pair list, table or output", who);
    if (n > 0 && nnz > 0 && (!col || !val)) return fail(NCF_EINVAL, "%s: %lld entries without col / val", who, (long long)nnz);
    if (n == 0) return NCF_OK;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return fail(NCF_EUNSUPPORTED, "%s: %lld pairs", who, (long long)n);
    hipLaunchKernelGGL(knn_predict_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, nnz, R, users, items, n,
                       nb_pos, nb_sim, nb_cnt, I, N, weighted_average, fill, out, dev_oob_flag);
    return check_launch(who);
}
