// Diversified top-K for gfx950: greedy Maximal Marginal Relevance over a pool of candidates per user (ncf_mmr_rerank, THE CONTRACT in
// include/ncf_abi.h).  A pool is what top_k_items / content_cosine_top_k return: N (score, item position) slots, of which the
// kernel picks K one after the other, each pick the slot whose  lambda * relevance - (1 - lambda) * (largest similarity to a slot
// already picked)  is largest.
//
// One workgroup per user, one thread per pool slot (64 * ceil(N / 64) threads).  A thread keeps its slot's relevance, its running
// maximum m_j and whether it can still be picked in registers.  The vector rows of the pool are gathered ONCE through the checked
// positions into LDS (row stride D + 1 words: thread-per-row reads of column d touch 32 different banks; all threads fill the image,
// 16 bytes per read, four reads in flight per thread), as many rows as fit in
// the 160 KiB beside the per-slot state (all of them unless N * (D + 1) words is more: N = 256 with D > 156); a slot past that
// reads its row from global memory (L2) at every step, 16 bytes at a time.  A step is
//     arg-max of the values   (butterfly inside each wave, then every thread folds the <= 4 wave winners read from LDS)
//     the pick's row copied to a 16-byte aligned LDS row, read back as broadcasts of 4 columns
//     sim(j, pick) by every thread that can still be picked, sequentially over d: that is K * n * D multiply-adds per user, where
//     the Gram matrix would be n * n * D
// with two workgroup barriers.  No atomics; nothing depends on timing: equal inputs give equal bits.
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py EXTRA_FLAGS): the contract rounds every product and every sum on its own.
// The pragma below says the same to a build that forgets the flag.
#include "ncf_common.h"
#include <math.h>

#pragma clang fp contract(off)

#define NCF_MMR_MAX_N 256
#define NCF_MMR_MAX_D 256
#define NCF_MMR_MAX_K 128
#define NCF_MMR_LDS_BYTES (160 * 1024)
#define NCF_MMR_MAXBLOCKS (1 << 20)

namespace ncf {

// a (value av, slot as) beats b: THE CONTRACT's comparator; a slot < 0 is "nothing" and loses to everything
__device__ __forceinline__ bool mmr_beats(float av, int as, float bv, int bs) {
    if (as < 0) return false;
    if (bs < 0) return true;
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an == bn ? as < bs : bn;
    return av > bv || (av == bv && as < bs);
}

// fixed LDS in front of the staged rows, in bytes (all carve offsets multiples of 16)
__host__ __device__ inline int mmr_fixed_bytes(int N, int D) { return D * 4 + ((N * 8 + 15) & ~15) + 64; }

template <bool VEC>
__global__ __launch_bounds__(256) void mmr_kernel(const float* __restrict__ vec, int64_t n_items, int D, int64_t ldv,
                                                  const float* __restrict__ score, const int64_t* __restrict__ pos,
                                                  const int32_t* __restrict__ count, int64_t B, int N, int K, float lambda, int normalize,
                                                  int rows_cap, int32_t* __restrict__ out_slot, float* __restrict__ out_value,
                                                  int32_t* __restrict__ out_count, int32_t* oob) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* prow = reinterpret_cast<float*>(smem);                                  // the last pick's row, D floats
    int64_t* spos = reinterpret_cast<int64_t*>(smem + D * 4);                      // checked position of a slot, -1 where dead
    float* red_v = reinterpret_cast<float*>(smem + D * 4 + ((N * 8 + 15) & ~15));  // [0..3] wave winners' values / minima
    int* red_s = reinterpret_cast<int*>(red_v + 4);                                // [0..3] wave winners' slots
    float* red_h = red_v + 8;                                                      // [0..3] wave maxima
    int* red_c = reinterpret_cast<int*>(red_v + 12);                               // [0..3] live slots per wave
    float* rows = reinterpret_cast<float*>(smem + mmr_fixed_bytes(N, D));          // staged rows, stride D + 1
    const int j = threadIdx.x;
    const int lane = j & 63, wv = j >> 6, nw = blockDim.x >> 6;
    const int RS = D + 1;
    const float one_minus = 1.0f - lambda;
    const float ninf = -INFINITY;

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        int n = N;
        if (count) {
            n = count[b];
            n = n < 0 ? 0 : (n > N ? N : n);
        }
        // ---- the slot: checked before it is used as an address
        float sc = 0.f;
        int64_t p = -1;
        bool live = false;
        if (j < n) {
            p = pos[b * N + j];
            sc = score[b * N + j];
            const bool in = p >= 0 && p < n_items;
            if (!in && p != -1 && oob) *oob = 1;
            live = in && fabsf(sc) < INFINITY;                 // false for NaN and +-inf
            if (!live) p = -1;
        }
        if (j < N) spos[j] = p;
        // ---- live count, and min / max of the live scores
        float lo = live ? sc : INFINITY, hi = live ? sc : -INFINITY;
        int c = live ? 1 : 0;
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
            c += __shfl_xor(c, o, 64);
        }
        if (lane == 0) {
            red_v[wv] = lo;
            red_h[wv] = hi;
            red_c[wv] = c;
        }
        __syncthreads();
        lo = red_v[0];
        hi = red_h[0];
        c = red_c[0];
        for (int w = 1; w < nw; ++w) {
            lo = fminf(lo, red_v[w]);
            hi = fmaxf(hi, red_h[w]);
            c += red_c[w];
        }
        const int n_out = c < K ? c : K;
        float rel = sc;
        if (normalize) {
            const float range = hi - lo;
            const float num = sc - lo;
            rel = hi == lo ? 0.f : num / range;
        }
        // ---- the pool's rows into LDS: the image is cut into pieces of 16 bytes (VEC) or single floats that the threads take in turn,
        // four pieces requested per thread before the first is stored (a wave has nothing else to hide the reads behind)
        const int n_staged = n < rows_cap ? n : rows_cap;
        {
            constexpr int W = VEC ? 4 : 1;
            const int ppr = D / W;                             // pieces per row
            const int total = n_staged * ppr;
            const int step = (int)blockDim.x;
            for (int c0 = j; c0 < total; c0 += 4 * step) {
                float q[4][W];
                int at[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * step;
                    at[u] = -1;
                    if (c < total) {
                        const int r = c / ppr, col = (c - r * ppr) * W;
                        const int64_t pr = spos[r];            // written before the barrier above
                        if (pr >= 0) {                         // a dead slot's row is never read
                            at[u] = r * RS + col;
                            const float* src = vec + pr * ldv + col;
                            if constexpr (VEC) {
                                const f32x4 x = *reinterpret_cast<const f32x4*>(src);
                                q[u][0] = x.x; q[u][1] = x.y; q[u][2] = x.z; q[u][3] = x.w;
                            } else {
                                q[u][0] = *src;
                            }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (at[u] >= 0) {
#pragma unroll
                        for (int k = 0; k < W; ++k) rows[at[u] + k] = q[u][k];
                    }
            }
        }
        float m = ninf;
        bool open = live;                                      // live and not picked yet
        const float lrel = lambda * rel;
        for (int t = 0; t < n_out; ++t) {
            // ---- value and arg-max
            float v = t == 0 ? rel : lrel - one_minus * m;
            int s = open ? j : -1;
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int os = __shfl_xor(s, o, 64);
                if (mmr_beats(ov, os, v, s)) {
                    v = ov;
                    s = os;
                }
            }
            __syncthreads();                                   // the staged rows (t == 0) and the last step's reads of red_* / prow are done
            if (lane == 0) {
                red_v[wv] = v;
                red_s[wv] = s;
            }
            __syncthreads();
            v = red_v[0];
            s = red_s[0];
            for (int w = 1; w < nw; ++w) {
                const float ov = red_v[w];
                const int os = red_s[w];
                if (mmr_beats(ov, os, v, s)) {
                    v = ov;
                    s = os;
                }
            }
            // s >= 0: t < n_out <= the number of live slots, and a step closes exactly one
            if (j == 0) {
                out_slot[b * K + t] = s;
                out_value[b * K + t] = v;
            }
            if (j == s) open = false;
            if (t + 1 == n_out) break;                         // the last pick changes nobody's value that is still read
            // ---- the pick's row, then the similarities to it
            const int64_t pp = spos[s];
            if (s < n_staged) {
                for (int d = j; d < D; d += blockDim.x) prow[d] = rows[s * RS + d];
            } else {
                for (int d = j; d < D; d += blockDim.x) prow[d] = vec[pp * ldv + d];
            }
            __syncthreads();
            if (open) {
                float acc = 0.f;
                if (j < n_staged) {
                    const float* r = rows + j * RS;
#pragma unroll 4                                               // 16 row reads and 4 broadcasts in flight: one wave per SIMD hides nothing
                    for (int d = 0; d < D; d += 4) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(prow + d);
                        acc = acc + r[d] * q.x;
                        acc = acc + r[d + 1] * q.y;
                        acc = acc + r[d + 2] * q.z;
                        acc = acc + r[d + 3] * q.w;
                    }
                } else {
                    const float* r = vec + p * ldv;
#pragma unroll 8                                               // 8 x 16 bytes of the row in flight per lane
                    for (int d = 0; d < D; d += 4) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(prow + d);
                        float a0, a1, a2, a3;
                        if (VEC) {
                            const f32x4 a = *reinterpret_cast<const f32x4*>(r + d);
                            a0 = a.x; a1 = a.y; a2 = a.z; a3 = a.w;
                        } else {
                            a0 = r[d]; a1 = r[d + 1]; a2 = r[d + 2]; a3 = r[d + 3];
                        }
                        acc = acc + a0 * q.x;
                        acc = acc + a1 * q.y;
                        acc = acc + a2 * q.z;
                        acc = acc + a3 * q.w;
                    }
                }
                if (acc > m) m = acc;
            }
        }
        if (j == 0) out_count[b] = n_out;
        if (j < K && j >= n_out) {
            out_slot[b * K + j] = -1;
            out_value[b * K + j] = ninf;
        }
        __syncthreads();                                       // the next user's slots overwrite spos / red_* / rows
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_mmr_supported(int N, int D, int K) {
    return N >= 1 && N <= NCF_MMR_MAX_N && D >= 4 && D <= NCF_MMR_MAX_D && D % 4 == 0 && K >= 1 && K <= NCF_MMR_MAX_K && K <= N ? 1 : 0;
}

extern "C" int ncf_mmr_rerank(const float* vec, int64_t n_items, int D, int64_t ldv, const float* score, const int64_t* pos,
                              const int32_t* count, int64_t B, int N, int K, float lambda, int normalize, int32_t* out_slot,
                              float* out_value, int32_t* out_count, int32_t* oob, ncf_stream_t stream) {
    if (B < 0 || n_items < 0 || N < 0 || D < 0 || K < 0)
        return fail(NCF_EINVAL, "ncf_mmr_rerank: negative size B=%lld n_items=%lld N=%d D=%d K=%d", (long long)B, (long long)n_items, N, D, K);
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail(NCF_EINVAL, "ncf_mmr_rerank: lambda = %g is outside [0, 1]", (double)lambda);
    if (normalize != 0 && normalize != 1) return fail(NCF_EINVAL, "ncf_mmr_rerank: normalize = %d is neither 0 nor 1", normalize);
    if (ldv < D) return fail(NCF_EINVAL, "ncf_mmr_rerank: leading dimension smaller than row (D=%d ldv=%lld)", D, (long long)ldv);
    if (B == 0) return NCF_OK;                                 // before any pointer is looked at
    if (!score || !pos || !out_slot || !out_value || !out_count || (n_items > 0 && !vec)) return fail(NCF_EINVAL, "ncf_mmr_rerank: null pointer");
    if (!ncf_mmr_supported(N, D, K))
        return fail(NCF_EUNSUPPORTED, "ncf_mmr_rerank: N=%d D=%d K=%d is outside 1 <= N <= %d, 4 <= D <= %d with D %% 4 == 0, 1 <= K <= min(N, %d)",
                    N, D, K, NCF_MMR_MAX_N, NCF_MMR_MAX_D, NCF_MMR_MAX_K);
    const int fixed = mmr_fixed_bytes(N, D);
    int rows_cap = (NCF_MMR_LDS_BYTES - fixed) / ((D + 1) * 4);
    if (rows_cap > N) rows_cap = N;
    const size_t lds = (size_t)fixed + (size_t)rows_cap * (D + 1) * 4;
    const bool v4 = ldv % 4 == 0 && aligned16(vec);
    const void* fn = v4 ? reinterpret_cast<const void*>(&mmr_kernel<true>) : reinterpret_cast<const void*>(&mmr_kernel<false>);
    if (lds > 65536 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, NCF_MMR_LDS_BYTES) != hipSuccess)
        return fail(NCF_ELAUNCH, "ncf_mmr_rerank: %zu bytes of LDS refused: %s", lds, hipGetErrorString(hipGetLastError()));
    const unsigned blocks = (unsigned)(B < NCF_MMR_MAXBLOCKS ? B : NCF_MMR_MAXBLOCKS);          // grid-stride beyond
    const unsigned threads = 64u * (unsigned)((N + 63) / 64);
    hipStream_t s = (hipStream_t)stream;
    if (v4)
        hipLaunchKernelGGL(mmr_kernel<true>, dim3(blocks), dim3(threads), lds, s, vec, n_items, D, ldv, score, pos, count, B, N, K, lambda,
                           normalize, rows_cap, out_slot, out_value, out_count, oob);
    else
        hipLaunchKernelGGL(mmr_kernel<false>, dim3(blocks), dim3(threads), lds, s, vec, n_items, D, ldv, score, pos, count, B, N, K, lambda,
                           normalize, rows_cap, out_slot, out_value, out_count, oob);
    return check_launch("ncf_mmr_rerank");
}
