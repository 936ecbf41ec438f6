// ImplicitALS, the implicit-feedback alternating-least-squares baseline (Hu, Koren & Volinsky 2008; implicit's
// AlternatingLeastSquares; the iALS of Rendle et al. 2021) on gfx950: the Gram matrix of a factor table, and one half-sweep
//     x_u = (G + sum_e (alpha v_e) t_e t_e^T + reg I)^-1  sum_e (1 + alpha v_e) t_e
// for listed rows of a ratings CSR, by Cholesky, WITHOUT float atomics and in one fixed order of every sum (THE CONTRACT in
// include/ncf_abi.h, restated in fp32 numpy by tests/als_ref.py).
//
// One workgroup of 256 threads owns one row.  The lower triangle of the F x F normal matrix is cut into nt x nt tiles of R x R
// elements (R = 1, 2, 4 or 8, the smallest with 16 R >= F; nt = ceil(F / R) <= 16) and the at most 136 tiles on or below the
// diagonal are dealt to the first threads of the workgroup, which keep their tile in registers from the first rank-1 update to the
// last elimination step.  T's rows of 16 entries at a time are staged in LDS; a rank-1 update reads 2 R floats of it for R * R
// multiply-adds.  The elimination is the blocked right-looking one: the diagonal tile of block J is factored in registers, the
// tiles below it are solved against it, every tile to the right subtracts the R columns of block J in ascending order.  Each
// element thus has the products of the contract subtracted from it one by one in ascending k: the blocking changes who computes,
// not what is computed.  L is left in an LDS tile, column by column, and one wave runs the two substitutions over it.
//
// A row longer than one segment of 512 entries has its segment sums S_s computed by one workgroup per segment (als_seg_kernel) into
// a scratch buffer; the row's workgroup adds them in segment order.  A short row computes its single S_0 itself: the same sums.
// The right-hand side b is one serial sum over all the row's entries by contract and stays in the row's own workgroup, which for
// such a row stages 64 entries a step (in the tile L does not occupy yet) and does nothing else while it streams.
//
// Every id is checked before it is used as an address; what the kernels refuse sets a bit of the sticky flag word.
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py EXTRA_FLAGS): every product, sum, quotient and square root of the contract is
// rounded on its own.  The pragma below says the same to a build that forgets the flag.  hipcc's default fp32 division and square
// root are correctly rounded and are relied on; no fast-math flag may be added to this file.
#include "ncf_common.h"

#include <math.h>

#pragma clang fp contract(off)

#define NCF_ALS_THREADS 256
#define NCF_ALS_STAGE 16                  // entries (rows of T) staged per step
#define NCF_ALS_STAGE_LONG 64             // ... by the own workgroup of a row of several segments, which only sums b: staged where L will be
#ifndef NCF_ALS_R8_BLOCKS
#define NCF_ALS_R8_BLOCKS 2               // workgroups per CU the solve kernel's registers are kept to: R = 8 (the LDS tile allows two)
#endif
#ifndef NCF_ALS_SMALL_BLOCKS
#define NCF_ALS_SMALL_BLOCKS 5            // ... and R < 8
#endif

namespace ncf {

struct AlsGeom {
    int R, nt, FP, LP;                    // tile edge, tiles per side, padded F (nt * R), row pitch of the L tile (FP + 1: odd, conflict free)
};

static AlsGeom als_geom(int F) {
    AlsGeom g;
    const int need = (F + 15) / 16;
    g.R = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
    g.nt = (F + g.R - 1) / g.R;
    g.FP = g.nt * g.R;
    g.LP = g.FP + 1;
    return g;
}

// thread t -> tile (ty, tx), tx <= ty, row-major over the triangle; false beyond the last tile
__device__ __forceinline__ bool als_tile_of(int t, int nt, int& ty, int& tx) {
    int row = 0, start = 0;
    while (row < nt && t >= start + row + 1) {
        start += row + 1;
        ++row;
    }
    ty = row;
    tx = t - start;
    return row < nt;
}

// acc[i][k] = acc[i][k] + (w * t[a]) * t[b]   (gram: t[a] * t[b]) for the tile's a = ty R + i, b = tx R + k
template <int R, bool GRAM>
__device__ __forceinline__ void als_rank1(float (&acc)[R][R], const float* __restrict__ trow, float w, int ty, int tx) {
    float ta[R], tb[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        ta[i] = trow[ty * R + i];
        tb[i] = trow[tx * R + i];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float wa = GRAM ? ta[i] : w * ta[i];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float p = wa * tb[k];
            acc[i][k] = acc[i][k] + p;
        }
    }
}

// Stages the entries [e0, e0 + nb) of a row that begins at row_beg, nb <= 4 kPer: wave w loads entries w, w + 4, w + 8, ..., all their
// columns and values first and then all their rows of T, so that a step waits for two memory round trips and not for 2 kPer.  st: T's row, zero
// beyond F; sw: alpha * val; sok: whether the entry counts.  FLAGS: the row's own workgroup also reports what it skips and checks
// the order of the columns.
template <bool FLAGS, int kPer>
__device__ __forceinline__ void als_stage_entries(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t e0, int nb,
                                                  int64_t row_beg, const float* __restrict__ T, int64_t n_t, int64_t ldt, int F, int FP,
                                                  float alpha, float* st, float* sw, int* sok, int32_t* flag, int* s_bad) {
    constexpr int kWaves = NCF_ALS_THREADS / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    static_assert(NCF_ALS_MAX_FACTORS <= 128, "a lane stages two floats of a row");
    int c[kPer], prev[kPer];
    float v[kPer];
    bool ok[kPer], after[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = wave + q * kWaves;
        const int64_t e = e0 + j;
        const bool live = j < nb;
        c[q] = live ? col[e] : -1;
        v[q] = live ? val[e] : -1.0f;
        after[q] = FLAGS && live && e > row_beg;
        prev[q] = after[q] ? col[e - 1] : 0;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = wave + q * kWaves;
        const bool okc = c[q] >= 0 && (int64_t)c[q] < n_t;
        const bool okv = v[q] >= 0.0f && v[q] < INFINITY;  // false for a NaN
        ok[q] = j < nb && okc && okv;
        if (j < nb && lane == 0) {
            if (FLAGS) {
                int bits = (okc ? 0 : NCF_ALS_FLAG_COL) | (okv ? 0 : NCF_ALS_FLAG_VAL);
                if (after[q] && prev[q] >= c[q]) {
                    bits |= NCF_ALS_FLAG_ORDER;
                    *s_bad = 1;
                }
                if (bits && flag) atomicOr(flag, bits);
            }
            sw[j] = alpha * v[q];
            sok[j] = ok[q] ? 1 : 0;
        }
    }
    float tv[kPer][2];                                     // FP <= 128: a lane holds at most two floats of a row
#pragma unroll
    for (int q = 0; q < kPer; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int a = lane + 64 * h;
            tv[q][h] = ok[q] && a < F ? T[(int64_t)c[q] * ldt + a] : 0.0f;
        }
#pragma unroll
    for (int q = 0; q < kPer; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int a = lane + 64 * h;
            if (ok[q] && a < FP) st[(wave + q * kWaves) * FP + a] = tv[q][h];
        }
}

// the lower triangle of a tile to a (F, F) matrix in global memory
template <int R>
__device__ __forceinline__ void als_store_tile(const float (&acc)[R][R], float* __restrict__ dst, int F, int ty, int tx) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int a = ty * R + i, b = tx * R + k;
            if (a < F && b <= a) dst[(int64_t)a * F + b] = acc[i][k];
        }
}

// P_c of the contract: one workgroup per chunk of 256 rows
template <int R>
__global__ __launch_bounds__(NCF_ALS_THREADS) void als_gram_chunk_kernel(const float* __restrict__ T, int64_t rows, int64_t ld, int F, int nt,
                                                                          float* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char als_lds[];
    float* st = reinterpret_cast<float*>(als_lds);
    const int FP = nt * R;
    int ty, tx;
    const bool tile = als_tile_of(threadIdx.x, nt, ty, tx);
    float acc[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = 0; k < R; ++k) acc[i][k] = 0.0f;
    const int64_t r0 = (int64_t)blockIdx.x * NCF_ALS_GRAM_ROWS;
    const int64_t r1 = r0 + NCF_ALS_GRAM_ROWS < rows ? r0 + NCF_ALS_GRAM_ROWS : rows;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t q0 = r0; q0 < r1; q0 += NCF_ALS_STAGE) {
        const int nb = (int)(r1 - q0 < NCF_ALS_STAGE ? r1 - q0 : NCF_ALS_STAGE);
        __syncthreads();                                   // the step before has been read
        for (int j = wave; j < nb; j += NCF_ALS_THREADS / 64) {
            const float* trow = T + (q0 + j) * ld;
            for (int a = lane; a < FP; a += 64) st[j * FP + a] = a < F ? trow[a] : 0.0f;
        }
        __syncthreads();
        if (tile)
            for (int j = 0; j < nb; ++j) als_rank1<R, true>(acc, st + j * FP, 0.0f, ty, tx);
    }
    if (tile) als_store_tile<R>(acc, part + (int64_t)blockIdx.x * F * F, F, ty, tx);
}

// G = the chunks added in ascending order, mirrored: one lane per element of the lower triangle
__global__ __launch_bounds__(256) void als_gram_sum_kernel(const float* __restrict__ part, int64_t chunks, int F, float* __restrict__ G) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * F) return;
    const int a = idx / F, b = idx % F;
    if (b > a) return;
    float g = 0.0f;
    for (int64_t c = 0; c < chunks; ++c) g = g + part[c * F * F + idx];
    G[a * F + b] = g;
    G[b * F + a] = g;
}

// S_s of the contract for one scratch slot: one workgroup per (listed row, segment) of the plan
template <int R>
__global__ __launch_bounds__(NCF_ALS_THREADS) void als_seg_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t nR,
    const int64_t* __restrict__ rows, int64_t B, const float* __restrict__ T, int64_t n_t, int64_t ldt, int F, int nt, float alpha,
    const int64_t* __restrict__ seg_base, const int64_t* __restrict__ seg_row, int64_t n_slots, float* __restrict__ scratch) {
    extern __shared__ __align__(16) unsigned char als_lds[];
    const int FP = nt * R;
    float* st = reinterpret_cast<float*>(als_lds);
    float* sw = st + NCF_ALS_STAGE * FP;
    int* sok = reinterpret_cast<int*>(sw + NCF_ALS_STAGE);
    const int64_t slot = blockIdx.x;
    // everything below is uniform over the workgroup; a slot the plan does not place is left alone (the row's workgroup reports it)
    const int64_t k = seg_row[slot];
    if (k < 0 || k >= B) return;
    const int64_t base = seg_base[k];
    if (base < 0 || base > slot) return;
    const int64_t s = slot - base;
    const int64_t row = rows[k];
    if (row < 0 || row >= nR) return;
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    if (beg < 0 || end > nnz || end < beg) return;
    if (s >= (end - beg + NCF_ALS_SEG - 1) / NCF_ALS_SEG) return;
    const int64_t s0 = beg + s * NCF_ALS_SEG;
    const int64_t s1 = s0 + NCF_ALS_SEG < end ? s0 + NCF_ALS_SEG : end;
    int ty, tx;
    const bool tile = als_tile_of(threadIdx.x, nt, ty, tx);
    float acc[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int kk = 0; kk < R; ++kk) acc[i][kk] = 0.0f;
    for (int64_t e0 = s0; e0 < s1; e0 += NCF_ALS_STAGE) {
        const int nb = (int)(s1 - e0 < NCF_ALS_STAGE ? s1 - e0 : NCF_ALS_STAGE);
        __syncthreads();
        als_stage_entries<false, NCF_ALS_STAGE / 4>(col, val, e0, nb, beg, T, n_t, ldt, F, FP, alpha, st, sw, sok, nullptr, nullptr);
        __syncthreads();
        if (tile)
            for (int j = 0; j < nb; ++j)
                if (sok[j]) als_rank1<R, false>(acc, st + j * FP, sw[j], ty, tx);
    }
    if (tile) als_store_tile<R>(acc, scratch + slot * F * F, F, ty, tx);
}

__device__ __forceinline__ void als_zero_row(float* __restrict__ orow, int F) {
    for (int a = threadIdx.x; a < F; a += NCF_ALS_THREADS) orow[a] = 0.0f;
}

// One listed row per workgroup: S (or the segments of the scratch buffer), A, b, Cholesky, the substitutions.  The second launch
// bound keeps the registers to what lets two workgroups (R = 8: the LDS tile allows no more) or five share a CU.
template <int R>
__global__ __launch_bounds__(NCF_ALS_THREADS, R == 8 ? NCF_ALS_R8_BLOCKS : NCF_ALS_SMALL_BLOCKS) void als_solve_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t nR,
    const int64_t* __restrict__ rows, int64_t B, const float* __restrict__ T, int64_t n_t, int64_t ldt, int F, int nt,
    const float* __restrict__ G, float alpha, float reg, float* __restrict__ out, int64_t ldo, int out_by_row,
    const int64_t* __restrict__ seg_base, const int64_t* __restrict__ seg_row, int64_t n_slots, const float* __restrict__ scratch,
    int32_t* flag) {
    extern __shared__ __align__(16) unsigned char als_lds[];
    const int FP = nt * R, LP = FP + 1;
    float* Ls = reinterpret_cast<float*>(als_lds);                     // Ls[j * LP + i] = L[i][j]: column j of L, contiguous
    float* st = Ls + FP * LP;
    float* sw = st + NCF_ALS_STAGE * FP;                               // NCF_ALS_STAGE_LONG floats
    float* sb = sw + NCF_ALS_STAGE_LONG;                               // b, FP floats
    int* sok = reinterpret_cast<int*>(sb + FP);
    int* s_bad = sok + NCF_ALS_STAGE_LONG;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    // ---- the row: every test here is uniform over the workgroup, and comes before the first barrier
    const int64_t row = rows[k];
    if (row < 0 || row >= nR) {
        if (tid == 0 && flag) atomicOr(flag, NCF_ALS_FLAG_PTR);
        if (!out_by_row) als_zero_row(out + k * ldo, F);
        return;
    }
    float* orow = out + (out_by_row ? row : k) * ldo;
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    if (beg < 0 || end > nnz || end < beg) {
        if (tid == 0 && flag) atomicOr(flag, NCF_ALS_FLAG_PTR);
        als_zero_row(orow, F);
        return;
    }
    const int64_t n = end - beg;
    if (n == 0) {
        als_zero_row(orow, F);
        return;
    }
    const int64_t nseg = (n + NCF_ALS_SEG - 1) / NCF_ALS_SEG;
    int64_t base = -1;
    if (nseg > 1) {
        base = seg_base ? seg_base[k] : -1;
        bool held = seg_row && base >= 0 && base <= n_slots - nseg;
        for (int64_t s = 0; held && s < nseg; ++s) held = seg_row[base + s] == k;
        if (!held) {
            if (tid == 0 && flag) atomicOr(flag, NCF_ALS_FLAG_PTR);
            als_zero_row(orow, F);
            return;
        }
    }
    int ty, tx;
    const bool tile = als_tile_of(tid, nt, ty, tx);
    const int ba = tid - (NCF_ALS_THREADS - FP);                       // the last FP threads keep b: the tiles sit in the first ones
    const bool bthread = ba >= 0 && ba < F;
    if (tid == 0) *s_bad = 0;
    float acc[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int kk = 0; kk < R; ++kk) acc[i][kk] = 0.0f;
    float bacc = 0.0f;
    // ---- every entry once: b always, S_0 when the row is a single segment
    if (nseg == 1 || FP < NCF_ALS_STAGE_LONG) {
        for (int64_t e0 = beg; e0 < end; e0 += NCF_ALS_STAGE) {
            const int nb = (int)(end - e0 < NCF_ALS_STAGE ? end - e0 : NCF_ALS_STAGE);
            __syncthreads();                                           // the step before has been read (and s_bad cleared)
            als_stage_entries<true, NCF_ALS_STAGE / 4>(col, val, e0, nb, beg, T, n_t, ldt, F, FP, alpha, st, sw, sok, flag, s_bad);
            __syncthreads();
            for (int j = 0; j < nb; ++j) {
                if (!sok[j]) continue;
                const float w = sw[j];
                if (tile && nseg == 1) als_rank1<R, false>(acc, st + j * FP, w, ty, tx);
                if (bthread) {
                    const float w1 = 1.0f + w;
                    const float p = w1 * st[j * FP + ba];
                    bacc = bacc + p;
                }
            }
        }
    } else {                                                           // b alone: 64 entries a step, staged in the tile L is not in yet
        for (int64_t e0 = beg; e0 < end; e0 += NCF_ALS_STAGE_LONG) {
            const int nb = (int)(end - e0 < NCF_ALS_STAGE_LONG ? end - e0 : NCF_ALS_STAGE_LONG);
            __syncthreads();
            als_stage_entries<true, NCF_ALS_STAGE_LONG / 4>(col, val, e0, nb, beg, T, n_t, ldt, F, FP, alpha, Ls, sw, sok, flag, s_bad);
            __syncthreads();
            if (bthread) {                                             // no branch, so that the LDS reads of several entries are in flight
#pragma unroll 8
                for (int j = 0; j < nb; ++j) {
                    const float w1 = 1.0f + sw[j];
                    const float p = w1 * Ls[j * FP + ba];
                    const float next = bacc + p;
                    bacc = sok[j] ? next : bacc;                       // a skipped entry's slot holds an older row: computed, not taken
                }
            }
        }
    }
    __syncthreads();                                                   // the last step has been read before L is written over it
    if (bthread) sb[ba] = bacc;
    // ---- A = G, + S_s in ascending s, + reg on the diagonal; beyond F the identity, which the elimination passes through
    if (tile) {
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int kk = 0; kk < R; ++kk) {
                const int a = ty * R + i, b = tx * R + kk;
                const bool in = a < F && b <= a;
                float v = in ? G[a * F + b] : (a == b ? 1.0f : 0.0f);
                if (nseg == 1) {
                    v = v + acc[i][kk];
                } else if (in) {
                    for (int64_t s = 0; s < nseg; ++s) v = v + scratch[(base + s) * F * F + a * F + b];
                }
                if (in && a == b) v = v + reg;
                acc[i][kk] = v;
            }
    }
    // ---- blocked right-looking Cholesky: block J = columns J R .. J R + R - 1
    for (int J = 0; J < nt; ++J) {
        if (tile && ty == J && tx == J) {                              // the diagonal tile, in registers
            bool bad = false;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float s = acc[j][j];
                if (!(s > 0.0f && s < INFINITY)) bad = true;
                const float d = sqrtf(s);
                acc[j][j] = d;
#pragma unroll
                for (int i = j + 1; i < R; ++i) acc[i][j] = acc[i][j] / d;
#pragma unroll
                for (int i = j + 1; i < R; ++i)
#pragma unroll
                    for (int kk = j + 1; kk <= i; ++kk) {
                        const float p = acc[i][j] * acc[kk][j];
                        acc[i][kk] = acc[i][kk] - p;
                    }
            }
            if (bad) {
                *s_bad = 1;
                if (flag) atomicOr(flag, NCF_ALS_FLAG_PIVOT);
            }
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
                for (int i = j; i < R; ++i) Ls[(J * R + j) * LP + J * R + i] = acc[i][j];
        }
        __syncthreads();
        if (tile && tx == J && ty > J) {                               // the tiles below it: rows of L against the diagonal tile
            float d[R][R];
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
                for (int kk = 0; kk <= j; ++kk) d[j][kk] = Ls[(J * R + kk) * LP + J * R + j];
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    float v = acc[i][j];
#pragma unroll
                    for (int kk = 0; kk < j; ++kk) {
                        const float p = acc[i][kk] * d[j][kk];
                        v = v - p;
                    }
                    acc[i][j] = v / d[j][j];
                }
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
                for (int i = 0; i < R; ++i) Ls[(J * R + j) * LP + ty * R + i] = acc[i][j];
        }
        __syncthreads();
        if (tile && tx > J) {                                          // every tile to the right: the block's columns in ascending order
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float* lc = Ls + (J * R + j) * LP;
                float la[R], lb[R];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    la[i] = lc[ty * R + i];
                    lb[i] = lc[tx * R + i];
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int kk = 0; kk < R; ++kk) {
                        const float p = la[i] * lb[kk];
                        acc[i][kk] = acc[i][kk] - p;
                    }
            }
        }
    }
    __syncthreads();
    // ---- the substitutions, by wave 0: lane l holds elements l and l + 64
    if (tid >= 64) return;
    const int lane = tid;
    if (*s_bad) {
        for (int a = lane; a < F; a += 64) orow[a] = 0.0f;
        return;
    }
    float c0 = lane < F ? sb[lane] : 0.0f, c1 = lane + 64 < F ? sb[lane + 64] : 0.0f;
    for (int q = 0; q < F; ++q) {                                      // forward: z in place
        const float* lc = Ls + q * LP;
        const float cq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q < 64 ? c0 : c1), q & 63));
        const float z = cq / lc[q];
        if (q < 64) {
            if (lane == q) c0 = z;
            if (lane > q && lane < F) {
                const float p = lc[lane] * z;
                c0 = c0 - p;
            }
            if (lane + 64 < F) {
                const float p = lc[lane + 64] * z;
                c1 = c1 - p;
            }
        } else {
            if (lane + 64 == q) c1 = z;
            if (lane + 64 > q && lane + 64 < F) {
                const float p = lc[lane + 64] * z;
                c1 = c1 - p;
            }
        }
    }
    for (int q = F - 1; q >= 0; --q) {                                 // backward: x in place; L[q][i] = Ls[i * LP + q]
        const float cq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q < 64 ? c0 : c1), q & 63));
        const float x = cq / Ls[q * LP + q];
        if (q >= 64) {
            if (lane + 64 == q) c1 = x;
            if (lane + 64 < q) {
                const float p = Ls[(lane + 64) * LP + q] * x;
                c1 = c1 - p;
            }
            if (lane < F) {
                const float p = Ls[lane * LP + q] * x;
                c0 = c0 - p;
            }
        } else {
            if (lane == q) c0 = x;
            if (lane < q) {
                const float p = Ls[lane * LP + q] * x;
                c0 = c0 - p;
            }
        }
    }
    if (lane < F) orow[lane] = c0;
    if (lane + 64 < F) orow[lane + 64] = c1;
}

static size_t als_solve_lds(const AlsGeom& g) {
    return sizeof(float) * ((size_t)g.FP * g.LP + (size_t)NCF_ALS_STAGE * g.FP + NCF_ALS_STAGE_LONG + g.FP) + sizeof(int) * (NCF_ALS_STAGE_LONG + 4);
}
static size_t als_stage_lds(const AlsGeom& g) { return sizeof(float) * ((size_t)NCF_ALS_STAGE * g.FP + NCF_ALS_STAGE) + sizeof(int) * NCF_ALS_STAGE; }

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_als_gram_workspace_bytes(int64_t rows, int F) {
    if (rows <= 0 || F < 1 || F > NCF_ALS_MAX_FACTORS) return 0;
    return (size_t)((rows + NCF_ALS_GRAM_ROWS - 1) / NCF_ALS_GRAM_ROWS) * F * F * sizeof(float);
}

extern "C" int ncf_als_gram(const float* T, int64_t rows, int64_t ld, int F, float* G, void* workspace, size_t workspace_bytes,
                            ncf_stream_t stream) {
    const char* who = "ncf_als_gram";
    if (rows < 0) return fail(NCF_EINVAL, "%s: negative size rows=%lld", who, (long long)rows);
    if (F < 1 || F > NCF_ALS_MAX_FACTORS) return fail(NCF_EINVAL, "%s: F = %d factors (1 .. %d)", who, F, NCF_ALS_MAX_FACTORS);
    if (ld < F) return fail(NCF_EINVAL, "%s: ld = %lld < F = %d", who, (long long)ld, F);
    if (!G || (rows > 0 && !T)) return fail(NCF_EINVAL, "%s: null table or output", who);
    if (!aligned(T, 4) || !aligned(G, 4) || !aligned(workspace, 4)) return fail(NCF_EINVAL, "%s: a float array is not 4-byte aligned", who);
    const size_t need = ncf_als_gram_workspace_bytes(rows, F);
    if (need && (!workspace || workspace_bytes < need))
        return fail(NCF_EINVAL, "%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
    const AlsGeom g = als_geom(F);
    const int64_t chunks = (rows + NCF_ALS_GRAM_ROWS - 1) / NCF_ALS_GRAM_ROWS;
    if (chunks > 0x7fffffff) return fail(NCF_EUNSUPPORTED, "%s: %lld chunks", who, (long long)chunks);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (chunks) {
        const size_t lds = als_stage_lds(g);
#define NCF_ALS_GRAM(RR) hipLaunchKernelGGL(als_gram_chunk_kernel<RR>, dim3((unsigned)chunks), dim3(NCF_ALS_THREADS), lds, s, T, rows, ld, F, g.nt, part)
        switch (g.R) {
            case 1: NCF_ALS_GRAM(1); break;
            case 2: NCF_ALS_GRAM(2); break;
            case 4: NCF_ALS_GRAM(4); break;
            default: NCF_ALS_GRAM(8); break;
        }
#undef NCF_ALS_GRAM
        if (const int rc = check_launch(who)) return rc;
    }
    hipLaunchKernelGGL(als_gram_sum_kernel, dim3((unsigned)((F * F + 255) / 256)), dim3(256), 0, s, part, chunks, F, G);
    return check_launch(who);
}

extern "C" int ncf_als_solve_rows(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t R, const int64_t* rows,
                                  int64_t B, const float* T, int64_t n_t, int64_t ldt, int F, const float* G, float alpha, float reg,
                                  float* out, int64_t ldo, int out_by_row, const int64_t* seg_base, const int64_t* seg_row,
                                  int64_t n_slots, float* scratch, int32_t* flag, ncf_stream_t stream) {
    const char* who = "ncf_als_solve_rows";
    if (nnz < 0 || R < 0 || B < 0 || n_t < 0 || n_slots < 0)
        return fail(NCF_EINVAL, "%s: negative size nnz=%lld R=%lld B=%lld n_t=%lld n_slots=%lld", who, (long long)nnz, (long long)R, (long long)B,
                    (long long)n_t, (long long)n_slots);
    if (F < 1 || F > NCF_ALS_MAX_FACTORS) return fail(NCF_EINVAL, "%s: F = %d factors (1 .. %d)", who, F, NCF_ALS_MAX_FACTORS);
    if (ldt < F || ldo < F) return fail(NCF_EINVAL, "%s: ldt = %lld or ldo = %lld < F = %d", who, (long long)ldt, (long long)ldo, F);
    if (!(reg > 0.f) || !isfinite(reg)) return fail(NCF_EINVAL, "%s: reg must be finite and > 0", who);
    if (!(alpha >= 0.f) || !isfinite(alpha)) return fail(NCF_EINVAL, "%s: alpha must be finite and >= 0", who);
    if (out_by_row != 0 && out_by_row != 1) return fail(NCF_EINVAL, "%s: out_by_row = %d (0 or 1)", who, out_by_row);
    if (!aligned(val, 4) || !aligned(col, 4) || !aligned(T, 4) || !aligned(G, 4) || !aligned(out, 4) || !aligned(scratch, 4) ||
        !aligned(flag, 4))
        return fail(NCF_EINVAL, "%s: a float or int32 array is not 4-byte aligned", who);
    if (!aligned(rowptr, 8) || !aligned(rows, 8) || !aligned(seg_base, 8) || !aligned(seg_row, 8))
        return fail(NCF_EINVAL, "%s: an int64 array is not 8-byte aligned", who);
    if (B > 0 && (!rowptr || !rows || !G || !out)) return fail(NCF_EINVAL, "%s: null pointers, row list, Gram matrix or output", who);
    if (B > 0 && nnz > 0 && (!col || !val)) return fail(NCF_EINVAL, "%s: %lld entries without col / val", who, (long long)nnz);
    if (B > 0 && nnz > 0 && n_t > 0 && !T) return fail(NCF_EINVAL, "%s: null table", who);
    if (B > 0 && n_slots > 0 && (!seg_base || !seg_row || !scratch)) return fail(NCF_EINVAL, "%s: %lld scratch slots without a plan or a buffer", who, (long long)n_slots);
    if (B == 0) return NCF_OK;
    if (B > 0x7fffffff || n_slots > 0x7fffffff) return fail(NCF_EUNSUPPORTED, "%s: %lld rows, %lld slots in one call", who, (long long)B, (long long)n_slots);
    const AlsGeom g = als_geom(F);
    hipStream_t s = (hipStream_t)stream;
    const size_t lds_seg = als_stage_lds(g), lds = als_solve_lds(g);
#define NCF_ALS_SOLVE(RR)                                                                                                                     \
    do {                                                                                                                                      \
        static std::atomic<unsigned long long> done{0};                                                                                       \
        if (lds > 64 * 1024 && !raise_lds((const void*)als_solve_kernel<RR>, done))                                                           \
            return fail(NCF_EUNSUPPORTED, "%s: cannot reserve %zu bytes of LDS", who, lds);                                                   \
        if (n_slots)                                                                                                                          \
            hipLaunchKernelGGL(als_seg_kernel<RR>, dim3((unsigned)n_slots), dim3(NCF_ALS_THREADS), lds_seg, s, rowptr, col, val, nnz, R, rows, B, \
                               T, n_t, ldt, F, g.nt, alpha, seg_base, seg_row, n_slots, scratch);                                              \
        hipLaunchKernelGGL(als_solve_kernel<RR>, dim3((unsigned)B), dim3(NCF_ALS_THREADS), lds, s, rowptr, col, val, nnz, R, rows, B, T, n_t,  \
                           ldt, F, g.nt, G, alpha, reg, out, ldo, out_by_row, seg_base, seg_row, n_slots, scratch, flag);                      \
    } while (0)
    switch (g.R) {
        case 1: NCF_ALS_SOLVE(1); break;
        case 2: NCF_ALS_SOLVE(2); break;
        case 4: NCF_ALS_SOLVE(4); break;
        default: NCF_ALS_SOLVE(8); break;
    }
#undef NCF_ALS_SOLVE
    return check_launch(who);
}
