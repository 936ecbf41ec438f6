// EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"), the closed-form item-item baseline, on gfx950:
//     G = X^T X,   P = (G + lambda 1)^-1,   W[i][j] = -P[i][j] / P[j][j] (i != j), W[j][j] = 0,   score(u, j) = sum_i X[u][i] W[i][j].
//
// ncf_ease_gram is knn.hip's walk (gram_walk.h) with the Gram row itself as its epilogue: no float atomics, one fixed order.
//
// ncf_ease_invert is a blocked, right-looking Gauss-Jordan inversion in place, without pivoting (every Schur complement of an SPD
// matrix is SPD), panel width NCF_EASE_BLOCK.  For the panel K = [k0, k0 + nb):
//     D   = A[K][K]^-1                                       one workgroup, the block in LDS (ease_diag_kernel)
//     R   = D * (A[K][:] with the columns K replaced by 1)   (nb, N)      \  ease_panel_kernel: a tiled GEMM and a transposed copy,
//     C^T = -(A[:][K] with the rows K replaced by -1)        (nb, N)      /  both into the workspace
//     A   = (A with the rows K and the columns K zeroed) + C^T^T * R      ease_update_kernel: ONE uniform rank-nb update of the whole
//                                                                          matrix, which also leaves R in the rows K, -A[:][K] D in
//                                                                          the columns K and D in the block (K, K)
// Both GEMMs are 128 x 128 tiles on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain), operands staged through LDS 32 k at
// a time, four independent 32 x 32 accumulators per wave, the next chunk's global loads in flight behind the MFMAs.  No split-K and
// no atomics: an entry's value is one chain over k in ascending order, whatever the grid.  2 N^3 FLOP in all.
//
// A pivot that is not positive and finite sets NCF_EASE_FLAG_PIVOT and a word in the workspace that every later launch of the call
// reads: from then on every update writes zeros, and as every update covers the whole matrix the output is all zeros.
//
// ncf_ease_weights / ncf_ease_scores / ncf_ease_predict are elementwise fp32 rules.  THIS FILE IS BUILT WITH -ffp-contract=off
// (build.py EXTRA_FLAGS): every product, sum and quotient of the contract (include/ncf_abi.h) is rounded on its own; the MFMA
// builtins are not touched by that flag.  hipcc's default fp32 division is correctly rounded and is relied on; no fast-math flag may
// be added to this file.
#include "ncf_common.h"
#include "gram_walk.h"

#include <math.h>

#pragma clang fp contract(off)

#define NCF_EASE_GRAM_TILE 2048           // columns per tile of a Gram row: 4 bytes of LDS each
#define NCF_EASE_TILE 128                 // output tile of the GEMMs: 128 x 128, four waves of 64 x 64
#define NCF_EASE_KC 32                    // k per staged chunk
#define NCF_EASE_LDS_LD 160               // floats per staged k row: 128 + 32, so rows k and k + 1 of one MFMA read lie 32 banks apart
#define NCF_EASE_DIAG_THREADS 1024
#define NCF_EASE_DEFAULT_STAGE 2048       // entries of a user's row staged in LDS by ncf_ease_scores (8 bytes each), as ncf_knn_scores
#define NCF_EASE_MAX_STAGE 8192
#define NCF_EASE_SCORE_THREADS 256
#define NCF_EASE_SCORE_COLS 4             // columns per lane of ncf_ease_scores: a tile is 1024 columns

static_assert(NCF_EASE_BLOCK == NCF_EASE_TILE, "a panel is one tile deep: the workspace rows are padded to the tile");
static_assert(NCF_EASE_BLOCK % NCF_EASE_KC == 0, "a panel is a whole number of chunks");

namespace ncf {

// ------------------------------------------------------------------------------------------------ Gram
// One (item, column tile) per one-wave workgroup: blockIdx.x = tile, blockIdx.y = item - i0.
__global__ __launch_bounds__(64) void ease_gram_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t U,
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ row, const float* __restrict__ tval, int64_t nnzT, int64_t I,
    int64_t i0, int T, float* __restrict__ out, int64_t ldg, int32_t* oob, int32_t* order) {
    extern __shared__ __align__(16) unsigned char ease_lds[];
    float* dot = reinterpret_cast<float*>(ease_lds);
    const int tile = blockIdx.x;
    const int64_t i = i0 + blockIdx.y;
    const int64_t t0 = (int64_t)tile * T;
    const int64_t t1 = t0 + T < I ? t0 + T : I;
    gram_row_walk<false>(rowptr, col, val, nnz, U, colptr, row, tval, nnzT, I, i, tile, t0, t1, dot, nullptr, oob, order);
    float* orow = out + (int64_t)blockIdx.y * ldg;
    for (int j = threadIdx.x; j < (int)(t1 - t0); j += 64) orow[t0 + j] = dot[j];
}

// ------------------------------------------------------------------------------------------------ inversion
// The workspace of one call: the `dead` word (256 bytes), D^T (nb x nb), C^T and R (nb rows of ldw floats each, ldw = N rounded up to
// the tile, so a tile's operand loads need no bounds).
struct EaseWs {
    int32_t* dead;
    float* dinvT;
    float* negCT;
    float* R;
    int64_t ldw;
};
__host__ __device__ inline int64_t ease_ldw(int64_t N) { return (N + NCF_EASE_TILE - 1) / NCF_EASE_TILE * NCF_EASE_TILE; }
static inline size_t ease_ws_bytes(int64_t N) {
    return 256 + sizeof(float) * ((size_t)NCF_EASE_BLOCK * NCF_EASE_BLOCK + 2 * (size_t)NCF_EASE_BLOCK * (size_t)ease_ldw(N));
}
static inline EaseWs ease_ws(void* p, int64_t N) {
    EaseWs w;
    w.dead = reinterpret_cast<int32_t*>(p);
    w.dinvT = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(p) + 256);
    w.ldw = ease_ldw(N);
    w.negCT = w.dinvT + (size_t)NCF_EASE_BLOCK * NCF_EASE_BLOCK;
    w.R = w.negCT + (size_t)NCF_EASE_BLOCK * w.ldw;
    return w;
}

// A[i][i] = A[i][i] + lambda, and the call's `dead` word cleared
__global__ __launch_bounds__(256) void ease_shift_kernel(float* __restrict__ A, int64_t N, int64_t lda, float lam, int32_t* dead) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *dead = 0;
    if (i < N) A[i * lda + i] = A[i * lda + i] + lam;
}

// D = A[K][K]^-1 by Gauss-Jordan without pivoting, in LDS, one workgroup; D^T goes to the workspace, zero-padded to nb x nb.
// Step k: p = a[k][k];  rowk[j] = a[k][j] / p (j != k), rowk[k] = 1 / p;  colk[i] = a[i][k];  then
//     a[k][j] = rowk[j];   a[i][k] = -(colk[i] * rowk[k]) (i != k);   a[i][j] = a[i][j] - colk[i] * rowk[j] (i != k, j != k).
__global__ __launch_bounds__(NCF_EASE_DIAG_THREADS) void ease_diag_kernel(const float* __restrict__ A, int64_t lda, int64_t k0, int bw,
                                                                         float* __restrict__ dinvT, int32_t* dead, int32_t* flag) {
    extern __shared__ __align__(16) unsigned char ease_lds[];
    constexpr int NB = NCF_EASE_BLOCK;
    float* a = reinterpret_cast<float*>(ease_lds);          // [NB][NB]
    float* rowk = a + NB * NB;
    float* colk = rowk + NB;
    const int t = threadIdx.x;
    for (int idx = t; idx < NB * NB; idx += NCF_EASE_DIAG_THREADS) {
        const int i = idx / NB, j = idx % NB;
        a[idx] = (i < bw && j < bw) ? A[(k0 + i) * lda + (k0 + j)] : 0.0f;
    }
    __syncthreads();
    bool bad = *dead != 0;                                   // uniform
    for (int k = 0; k < bw && !bad; ++k) {
        const float p = a[k * NB + k];                       // every thread reads the same word
        if (!(p > 0.0f) || !isfinite(p)) {
            bad = true;
            break;
        }
        if (t < NB) {
            rowk[t] = t == k ? 1.0f / p : a[k * NB + t] / p;
        } else if (t < 2 * NB) {
            colk[t - NB] = a[(t - NB) * NB + k];
        }
        __syncthreads();
        const int j = t % NB;                                // a thread keeps its column: rowk[j] and rowk[k] are read once per step
        if (j < bw) {
            const float rj = rowk[j], rk = rowk[k];
            for (int i = t / NB; i < bw; i += NCF_EASE_DIAG_THREADS / NB) {
                float v;
                if (i == k) {
                    v = rj;
                } else if (j == k) {
                    const float m = colk[i] * rk;
                    v = -m;
                } else {
                    const float m = colk[i] * rj;
                    v = a[i * NB + j] - m;
                }
                a[i * NB + j] = v;
            }
        }
        __syncthreads();
    }
    if (bad) {
        if (t == 0) {
            *dead = 1;
            if (flag) atomicOr(flag, NCF_EASE_FLAG_PIVOT);
        }
        for (int idx = t; idx < NB * NB; idx += NCF_EASE_DIAG_THREADS) dinvT[idx] = 0.0f;
        return;
    }
    for (int idx = t; idx < NB * NB; idx += NCF_EASE_DIAG_THREADS) {
        const int m = idx / NB, k = idx % NB;                // dinvT[m][k] = D[k][m]; lanes along k read a column of a: one bank apart + NB
        dinvT[idx] = a[k * NB + m];
    }
}

// acc[tm][tn] (+)= sum over k < 32 * chunks of Aop(k, i) * Bop(k, j) for the wave's 64 x 64 quarter of a 128 x 128 tile.  loadA / loadB:
// (k, c) -> the four operand values (k, c .. c + 3), c a multiple of 4 inside the tile; the chunk after the one being multiplied is in
// flight in registers.  Lane l of v_mfma_f32_32x32x2_f32 supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].
template <class LoadA, class LoadB>
__device__ __forceinline__ void ease_gemm_tile(f32x16 (&acc)[2][2], int chunks, LoadA loadA, LoadB loadB, float* As, float* Bs) {
    constexpr int LD = NCF_EASE_LDS_LD, KC = NCF_EASE_KC;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, l31 = lane & 31, h = lane >> 5;
    f32x4 pa[4], pb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = t + 256 * q;
        pa[q] = loadA(idx >> 5, (idx & 31) * 4);
        pb[q] = loadB(idx >> 5, (idx & 31) * 4);
    }
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();                                     // the last chunk's reads before this one's writes
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = t + 256 * q;
            *reinterpret_cast<f32x4*>(As + (idx >> 5) * LD + (idx & 31) * 4) = pa[q];
            *reinterpret_cast<f32x4*>(Bs + (idx >> 5) * LD + (idx & 31) * 4) = pb[q];
        }
        __syncthreads();
        if (c + 1 < chunks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = t + 256 * q;
                pa[q] = loadA((c + 1) * KC + (idx >> 5), (idx & 31) * 4);
                pb[q] = loadB((c + 1) * KC + (idx >> 5), (idx & 31) * 4);
            }
        }
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const float a0 = As[(kk + h) * LD + wm + l31], a1 = As[(kk + h) * LD + wm + 32 + l31];
            const float b0 = Bs[(kk + h) * LD + wn + l31], b1 = Bs[(kk + h) * LD + wn + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// One 128-column strip of the panel's two operands per workgroup: blockIdx.x = strip.  R = D * E over the strip (E: the rows K of A,
// with 1 on the columns K and 0 past N), all nb rows of it; and C^T over the same columns.  Rows past the panel's width are zeros.
__global__ __launch_bounds__(256, 2) void ease_panel_kernel(const float* __restrict__ A, int64_t N, int64_t lda, int64_t k0, int bw, EaseWs ws) {
    __shared__ __align__(16) float As[NCF_EASE_KC * NCF_EASE_LDS_LD];
    __shared__ __align__(16) float Bs[NCF_EASE_KC * NCF_EASE_LDS_LD];
    constexpr int NB = NCF_EASE_BLOCK;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * NCF_EASE_TILE;
    const bool dead = *ws.dead != 0;
    // C^T: lanes along i (coalesced stores), a lane reads its row of A along k
    {
        const int64_t i = j0 + (t & 127);
        const bool in_k = !dead && i >= k0 && i < k0 + bw;
        const bool load = !dead && i < N && !in_k;
        const float* arow = A + (load ? i * lda + k0 : 0);
#pragma unroll 8
        for (int k = (t >> 7) * (NB / 2); k < ((t >> 7) + 1) * (NB / 2); ++k) {
            float v = (in_k && i - k0 == k) ? 1.0f : 0.0f;
            if (load && k < bw) v = -arow[k];
            ws.negCT[(int64_t)k * ws.ldw + i] = v;
        }
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    const float* dinvT = ws.dinvT;
    auto loadA = [&](int m, int c) -> f32x4 { return *reinterpret_cast<const f32x4*>(dinvT + m * NB + c); };
    auto loadB = [&](int m, int c) -> f32x4 {
        f32x4 v;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t j = j0 + c + x;
            float e = 0.0f;
            if (m < bw && j < N) {
                if (j >= k0 && j < k0 + bw) e = (j - k0 == m) ? 1.0f : 0.0f;
                else e = A[(k0 + m) * lda + j];
            }
            v[x] = e;
        }
        return v;
    };
    ease_gemm_tile(acc, (bw + NCF_EASE_KC - 1) / NCF_EASE_KC, loadA, loadB, As, Bs);
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = wm + a * 32 + acc_row(r, h);
                ws.R[(int64_t)k * ws.ldw + j0 + wn + b * 32 + l31] = dead ? 0.0f : acc[a][b][r];
            }
}

// One 128 x 128 tile of the whole matrix per workgroup: blockIdx.x = column tile, blockIdx.y = row tile.
__global__ __launch_bounds__(256, 2) void ease_update_kernel(float* __restrict__ A, int64_t N, int64_t lda, int64_t k0, int bw, EaseWs ws) {
    __shared__ __align__(16) float As[NCF_EASE_KC * NCF_EASE_LDS_LD];
    __shared__ __align__(16) float Bs[NCF_EASE_KC * NCF_EASE_LDS_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, l31 = lane & 31, h = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.y * NCF_EASE_TILE, j0 = (int64_t)blockIdx.x * NCF_EASE_TILE;
    const int64_t k1 = k0 + bw;
    const bool dead = *ws.dead != 0;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + wn + b * 32 + l31;
            const bool jk = j >= N || (j >= k0 && j < k1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t i = i0 + wm + a * 32 + acc_row(r, h);
                const bool zero = dead || jk || i >= N || (i >= k0 && i < k1);
                acc[a][b][r] = zero ? 0.0f : A[i * lda + j];
            }
        }
    if (!dead) {
        const float* pa = ws.negCT + i0;
        const float* pb = ws.R + j0;
        const int64_t ldw = ws.ldw;
        auto loadA = [&](int k, int c) -> f32x4 { return *reinterpret_cast<const f32x4*>(pa + (int64_t)k * ldw + c); };
        auto loadB = [&](int k, int c) -> f32x4 { return *reinterpret_cast<const f32x4*>(pb + (int64_t)k * ldw + c); };
        ease_gemm_tile(acc, (bw + NCF_EASE_KC - 1) / NCF_EASE_KC, loadA, loadB, As, Bs);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + wn + b * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t i = i0 + wm + a * 32 + acc_row(r, h);
                if (i < N && j < N) A[i * lda + j] = acc[a][b][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------ weights
__global__ __launch_bounds__(256) void ease_diag_copy_kernel(const float* __restrict__ P, int64_t N, int64_t ldp, float* __restrict__ diag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) diag[i] = P[i * ldp + i];
}

// blockIdx.y = row (grid-stride), lanes along the columns
__global__ __launch_bounds__(256) void ease_weights_kernel(float* __restrict__ P, int64_t N, int64_t ldp, const float* __restrict__ diag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const float d = diag[j];
    for (int64_t i = blockIdx.y; i < N; i += gridDim.y) {
        const float q = P[i * ldp + j] / d;
        P[i * ldp + j] = i == j ? 0.0f : -q;
    }
}

// ------------------------------------------------------------------------------------------------ scores
// The score rule of the contract for C columns j0, j0 + stride, ... (those below j1) of one user row: cols / vals are the row's n
// entries, in LDS or in global memory.  A column id outside [0, I) sets the flag and adds nothing.
template <int C>
__device__ __forceinline__ void ease_score_cols(const int32_t* cols, const float* vals, int n, const float* __restrict__ W, int64_t ldw,
                                                int64_t I, int64_t j0, int64_t stride, int64_t j1, float (&s)[C], int32_t* oob) {
#pragma unroll
    for (int x = 0; x < C; ++x) s[x] = 0.0f;
    for (int e = 0; e < n; ++e) {
        const int c = cols[e];
        if (c < 0 || (int64_t)c >= I) {
            if (oob) atomicOr(oob, 1);
            continue;
        }
        const float v = vals[e];
        const float* wrow = W + (int64_t)c * ldw;
#pragma unroll
        for (int x = 0; x < C; ++x) {
            const int64_t j = j0 + x * stride;
            if (j < j1) {
                const float p = v * wrow[j];
                s[x] = s[x] + p;
            }
        }
    }
}

// One workgroup per (user, tile of 1024 columns): blockIdx.x = tile, blockIdx.y = user of the list.
__global__ __launch_bounds__(NCF_EASE_SCORE_THREADS) void ease_scores_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t R,
    const int64_t* __restrict__ users, const float* __restrict__ W, int64_t I, int64_t ldw, int64_t i0, int64_t i1, int stage_cap,
    float* __restrict__ out, int64_t ldo, int32_t* oob) {
    extern __shared__ __align__(16) unsigned char ease_lds[];
    int32_t* scol = reinterpret_cast<int32_t*>(ease_lds);
    float* sval = reinterpret_cast<float*>(ease_lds) + stage_cap;
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
        for (int e = threadIdx.x; e < n; e += NCF_EASE_SCORE_THREADS) {
            scol[e] = col[rb + e];
            sval[e] = val[rb + e];
        }
        __syncthreads();
    }
    const int64_t j0 = i0 + (int64_t)blockIdx.x * (NCF_EASE_SCORE_THREADS * NCF_EASE_SCORE_COLS) + threadIdx.x;
    if (j0 >= i1) return;
    float s[NCF_EASE_SCORE_COLS];
    if (staged)
        ease_score_cols<NCF_EASE_SCORE_COLS>(scol, sval, n, W, ldw, I, j0, NCF_EASE_SCORE_THREADS, i1, s, oob);
    else
        ease_score_cols<NCF_EASE_SCORE_COLS>(col + rb, val + rb, n, W, ldw, I, j0, NCF_EASE_SCORE_THREADS, i1, s, oob);
#pragma unroll
    for (int x = 0; x < NCF_EASE_SCORE_COLS; ++x) {
        const int64_t j = j0 + (int64_t)x * NCF_EASE_SCORE_THREADS;
        if (j < i1) out[b * ldo + (j - i0)] = s[x];
    }
}

// One lane per (user row, item) pair.
__global__ __launch_bounds__(256) void ease_predict_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, int64_t nnz, int64_t R,
    const int64_t* __restrict__ users, const int64_t* __restrict__ items, int64_t n_pairs, const float* __restrict__ W, int64_t I,
    int64_t ldw, float* __restrict__ out, int32_t* oob) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pairs) return;
    const int64_t u = users[k], i = items[k];
    float r[1] = {0.0f};                                   // what an empty row scores
    if (u < 0 || u >= R || i < 0 || i >= I) {
        if (oob) atomicOr(oob, 1);
    } else {
        int64_t rb, re;
        csr_range(rowptr, u, nnz, oob, rb, re);
        if (re - rb > 0x7fffffff) re = rb + 0x7fffffff;
        ease_score_cols<1>(col + rb, val + rb, (int)(re - rb), W, ldw, I, i, 0, I, r, oob);
    }
    out[k] = r[0];
}

static int ease_check_matrix(const char* who, const char* what, const void* p, int64_t N, int64_t ld) {
    if (N < 0) return fail(NCF_EINVAL, "%s: negative size N=%lld", who, (long long)N);
    if (ld < N) return fail(NCF_EINVAL, "%s: ld = %lld < N = %lld", who, (long long)ld, (long long)N);
    if (N > 65535) return fail(NCF_EUNSUPPORTED, "%s: N = %lld items (at most 65535)", who, (long long)N);
    if (N > 0 && !p) return fail(NCF_EINVAL, "%s: null %s", who, what);
    if (!aligned(p, 4)) return fail(NCF_EINVAL, "%s: %s is not 4-byte aligned", who, what);
    return NCF_OK;
}

static int ease_check_csr(const char* who, const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, bool touched) {
    if (touched && !rowptr) return fail(NCF_EINVAL, "%s: null row pointers", who);
    if (touched && nnz > 0 && (!col || !val)) return fail(NCF_EINVAL, "%s: %lld entries without col / val", who, (long long)nnz);
    if (!aligned(rowptr, 8) || !aligned(col, 4) || !aligned(val, 4)) return fail(NCF_EINVAL, "%s: a misaligned CSR array", who);
    return NCF_OK;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_ease_gram(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t U, const int64_t* colptr,
                             const int32_t* row, const float* tval, int64_t nnzT, int64_t I, int64_t i0, int64_t i1, float* G, int64_t ldg,
                             int32_t* dev_oob_flag, int32_t* dev_flag, ncf_stream_t stream) {
    const char* who = "ncf_ease_gram";
    if (U < 0 || I < 0 || nnz < 0 || nnzT < 0)
        return fail(NCF_EINVAL, "%s: negative size U=%lld I=%lld nnz=%lld nnzT=%lld", who, (long long)U, (long long)I, (long long)nnz, (long long)nnzT);
    if (i0 < 0 || i1 < i0 || i1 > I) return fail(NCF_EINVAL, "%s: items [%lld, %lld) outside [0, %lld)", who, (long long)i0, (long long)i1, (long long)I);
    if (ldg < I) return fail(NCF_EINVAL, "%s: ldg = %lld < I = %lld", who, (long long)ldg, (long long)I);
    if (I > 65535) return fail(NCF_EUNSUPPORTED, "%s: I = %lld items (at most 65535)", who, (long long)I);
    const bool work = i1 > i0;
    if (const int rc = ease_check_csr(who, rowptr, col, val, nnz, work)) return rc;
    if (const int rc = ease_check_csr(who, colptr, row, tval, nnzT, work)) return rc;
    if (work && !G) return fail(NCF_EINVAL, "%s: null output", who);
    if (!aligned(G, 4)) return fail(NCF_EINVAL, "%s: G is not 4-byte aligned", who);
    if (!work) return NCF_OK;
    const int64_t up = (I + 63) / 64 * 64;
    const int T = (int)(up < NCF_EASE_GRAM_TILE ? up : NCF_EASE_GRAM_TILE);
    const int64_t tiles = (I + T - 1) / T;
    hipLaunchKernelGGL(ease_gram_kernel, dim3((unsigned)tiles, (unsigned)(i1 - i0)), dim3(64), (size_t)T * 4, (hipStream_t)stream, rowptr, col,
                       val, nnz, U, colptr, row, tval, nnzT, I, i0, T, G, ldg, dev_oob_flag, dev_flag);
    return check_launch(who);
}

extern "C" size_t ncf_ease_invert_workspace_bytes(int64_t N) { return N <= 0 || N > 65535 ? 0 : ease_ws_bytes(N); }

extern "C" int ncf_ease_invert(float* A, int64_t N, int64_t lda, float lambda, void* workspace, size_t workspace_bytes, int32_t* dev_flag,
                               ncf_stream_t stream) {
    const char* who = "ncf_ease_invert";
    if (const int rc = ease_check_matrix(who, "matrix", A, N, lda)) return rc;
    if (!isfinite(lambda) || !(lambda > 0.f)) return fail(NCF_EINVAL, "%s: lambda must be finite and > 0", who);
    if (N == 0) return NCF_OK;
    if (!workspace || workspace_bytes < ease_ws_bytes(N))
        return fail(NCF_EINVAL, "%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, ease_ws_bytes(N));
    if (!aligned(workspace, 256)) return fail(NCF_EINVAL, "%s: workspace is not 256-byte aligned", who);
    const size_t diag_lds = sizeof(float) * (NCF_EASE_BLOCK * NCF_EASE_BLOCK + 2 * NCF_EASE_BLOCK);
    static std::atomic<unsigned long long> done{0};
    if (diag_lds > 64 * 1024 && !raise_lds((const void*)ease_diag_kernel, done))
        return fail(NCF_EUNSUPPORTED, "%s: cannot reserve %zu bytes of LDS", who, diag_lds);
    hipStream_t s = (hipStream_t)stream;
    const EaseWs ws = ease_ws(workspace, N);
    const unsigned tiles = (unsigned)(ws.ldw / NCF_EASE_TILE);
    hipLaunchKernelGGL(ease_shift_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, A, N, lda, lambda, ws.dead);
    for (int64_t k0 = 0; k0 < N; k0 += NCF_EASE_BLOCK) {
        const int bw = (int)(N - k0 < NCF_EASE_BLOCK ? N - k0 : NCF_EASE_BLOCK);
        hipLaunchKernelGGL(ease_diag_kernel, dim3(1), dim3(NCF_EASE_DIAG_THREADS), diag_lds, s, A, lda, k0, bw, ws.dinvT, ws.dead, dev_flag);
        hipLaunchKernelGGL(ease_panel_kernel, dim3(tiles), dim3(256), 0, s, A, N, lda, k0, bw, ws);
        hipLaunchKernelGGL(ease_update_kernel, dim3(tiles, tiles), dim3(256), 0, s, A, N, lda, k0, bw, ws);
    }
    return check_launch(who);
}

extern "C" int ncf_ease_weights(float* P, int64_t N, int64_t ldp, float* dev_diag, ncf_stream_t stream) {
    const char* who = "ncf_ease_weights";
    if (const int rc = ease_check_matrix(who, "matrix", P, N, ldp)) return rc;
    if (N > 0 && !dev_diag) return fail(NCF_EINVAL, "%s: null diagonal buffer", who);
    if (!aligned(dev_diag, 4)) return fail(NCF_EINVAL, "%s: the diagonal buffer is not 4-byte aligned", who);
    if (N == 0) return NCF_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ease_diag_copy_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, P, N, ldp, dev_diag);
    const unsigned rows = (unsigned)(N < 1024 ? N : 1024);
    hipLaunchKernelGGL(ease_weights_kernel, dim3((unsigned)((N + 255) / 256), rows), dim3(256), 0, s, P, N, ldp, dev_diag);
    return check_launch(who);
}

extern "C" int ncf_ease_scores(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t R, const int64_t* users,
                               int64_t B, const float* W, int64_t I, int64_t ldw, int64_t i0, int64_t i1, int stage_cap, float* out,
                               int64_t ldo, int32_t* dev_oob_flag, ncf_stream_t stream) {
    const char* who = "ncf_ease_scores";
    if (R < 0 || B < 0 || nnz < 0) return fail(NCF_EINVAL, "%s: negative size R=%lld B=%lld nnz=%lld", who, (long long)R, (long long)B, (long long)nnz);
    if (const int rc = ease_check_matrix(who, "weights", W, I, ldw)) return rc;
    if (i0 < 0 || i1 < i0 || i1 > I) return fail(NCF_EINVAL, "%s: items [%lld, %lld) outside [0, %lld)", who, (long long)i0, (long long)i1, (long long)I);
    if (stage_cap < 0 || stage_cap > NCF_EASE_MAX_STAGE) return fail(NCF_EINVAL, "%s: stage_cap = %d (0 .. %d)", who, stage_cap, NCF_EASE_MAX_STAGE);
    if (ldo < i1 - i0) return fail(NCF_EINVAL, "%s: ldo = %lld < %lld items", who, (long long)ldo, (long long)(i1 - i0));
    if (B > 65535) return fail(NCF_EUNSUPPORTED, "%s: %lld users in one call (at most 65535)", who, (long long)B);
    const bool work = B > 0 && i1 > i0;
    if (const int rc = ease_check_csr(who, rowptr, col, val, nnz, work)) return rc;
    if (work && (!users || !out)) return fail(NCF_EINVAL, "%s: null user list or output", who);
    if (!aligned(users, 8) || !aligned(out, 4)) return fail(NCF_EINVAL, "%s: a misaligned user list or output", who);
    if (!work) return NCF_OK;
    const int cap = stage_cap ? stage_cap : NCF_EASE_DEFAULT_STAGE;
    const int per = NCF_EASE_SCORE_THREADS * NCF_EASE_SCORE_COLS;
    const int64_t tiles = (i1 - i0 + per - 1) / per;
    hipLaunchKernelGGL(ease_scores_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(NCF_EASE_SCORE_THREADS), (size_t)cap * 8, (hipStream_t)stream,
                       rowptr, col, val, nnz, R, users, W, I, ldw, i0, i1, cap, out, ldo, dev_oob_flag);
    return check_launch(who);
}

extern "C" int ncf_ease_predict(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz, int64_t R, const int64_t* users,
                                const int64_t* items, int64_t n, const float* W, int64_t I, int64_t ldw, float* out, int32_t* dev_oob_flag,
                                ncf_stream_t stream) {
    const char* who = "ncf_ease_predict";
    if (R < 0 || n < 0 || nnz < 0) return fail(NCF_EINVAL, "%s: negative size R=%lld n=%lld nnz=%lld", who, (long long)R, (long long)n, (long long)nnz);
    if (const int rc = ease_check_matrix(who, "weights", W, I, ldw)) return rc;
    if (const int rc = ease_check_csr(who, rowptr, col, val, nnz, n > 0)) return rc;
    if (n > 0 && (!users || !items || !out)) return fail(NCF_EINVAL, "%s: null pair list or output", who);
    if (!aligned(users, 8) || !aligned(items, 8) || !aligned(out, 4)) return fail(NCF_EINVAL, "%s: a misaligned pair list or output", who);
    if (n == 0) return NCF_OK;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return fail(NCF_EUNSUPPORTED, "%s: %lld pairs", who, (long long)n);
    hipLaunchKernelGGL(ease_predict_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, nnz, R, users, items, n,
                       W, I, ldw, out, dev_oob_flag);
    return check_launch(who);
}
