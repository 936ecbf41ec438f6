// Row-sparse Adam (ncf_adam_rows): one Adam update of the embedding rows a batch touched, from the batch's per-occurrence
// gradient rows — no table-sized gradient buffer, no float atomics, no pass over untouched rows.
//
// Input: the batch's ids in ascending order (`ids`), the occurrence each sorted position came from (`perm`, NULL = identity)
// and the [n, E] gradient rows `g`.  A RUN is a maximal stretch of equal ids; its first position is its HEAD.  Every run is
// owned by exactly one worker, which adds the run's gradient rows and applies adam_update (adam_update.h, the function of
// the dense ncf_adam_step) to row `id` of p, m, v.  Rows of different runs are disjoint: no atomics, no races, and equal
// inputs give equal bits.
//
// Two kernels share the work by run length (kLongRun = 64; "long" <=> ids[head + 64] == ids[head]):
//   adam_rows_kernel       one 16-lane group per sorted position (4 runs per wave); a group whose position is no head, or the
//                          head of a long run, does nothing.  Lane l of the group owns the 16-byte chunks l, l + 16, ... of
//                          the row (single floats on the scalar path).
//   adam_rows_long_kernel  one 1024-thread workgroup per long run (a tile of 64 positions holds at most one long head, so a
//                          wave finds it with one ballot): its 64 groups add interleaved shares of the run, 8 independent
//                          row loads in flight per lane, and the shares are combined through LDS.  A batch in which one id is
//                          a quarter of 65 536 pairs is 32 such rounds per group, not 16 384 dependent loads of one wave.
//
// RUN-SUM ORDER (a fixed function of the sorted input; r = run length, x_k = g[perm[head + k]]):
//   r <= 64 :  ((x_0 + x_1) + x_2) + ... + x_{r-1}                               left to right in sorted order
//   r  > 64 :  S_q = ((x_q + x_{q+64}) + x_{q+128}) + ...   for q = 0 .. 63,     then  ((S_0 + S_1) + S_2) + ... + S_63
// (the long form starts each S_q from +0 and pads a share's last round with +0; neither changes a sum.)  perm comes from a
// STABLE sort in the binding, so the order is a function of the batch alone.  A run of one row is that row, bit for bit.
#include "ncf_common.h"
#include "adam_update.h"

namespace ncf {

constexpr int kRowGroup = 16;     // lanes that own one run in adam_rows_kernel
constexpr int kLongRun = 64;      // runs longer than this go to adam_rows_long_kernel
constexpr int kLongGroups = 64;   // 16-lane groups of its 1024-thread workgroup = interleaved shares of a long run
constexpr int kLongFlight = 8;    // independent row loads in flight per lane there

template <typename T> __device__ __forceinline__ T row_zero();
template <> __device__ __forceinline__ float row_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ f32x4 row_zero<f32x4>() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ void adam_update_chunk(float& p, float& m, float& v, float g, const AdamCoef& k) { adam_update(p, m, v, g, k); }
__device__ __forceinline__ void adam_update_chunk(f32x4& p, f32x4& m, f32x4& v, f32x4 g, const AdamCoef& k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_update(pj, mj, vj, g[j], k);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
    }
}

// T = f32x4 (16-byte path: E, ld, ld_g multiples of 4, 16-byte aligned bases) or float (any E >= 1).  W = chunks per row.
template <typename T>
__global__ __launch_bounds__(256) void adam_rows_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int64_t ld,
                                                        int64_t rows, int E, const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ perm, int64_t n, const float* __restrict__ g,
                                                        int64_t ld_g, AdamCoef k, int32_t* oob) {
    constexpr int V = sizeof(T) / 4;
    const int W = E / V;
    const int lig = threadIdx.x & (kRowGroup - 1);
    const int shift = (threadIdx.x & 63) & ~(kRowGroup - 1);         // this group's 16 bits of a wave ballot
    const int64_t groups = (int64_t)gridDim.x * (blockDim.x / kRowGroup);
    for (int64_t j = (int64_t)blockIdx.x * (blockDim.x / kRowGroup) + threadIdx.x / kRowGroup; j < n; j += groups) {
        // everything up to the chunk loop is uniform over the 16 lanes of the group
        const int64_t id = ids[j];
        if (j > 0 && ids[j - 1] == id) continue;                                  // not a head
        if (j + kLongRun < n && ids[j + kLongRun] == id) continue;                // a long run: adam_rows_long_kernel's
        if (id < 0 || id >= rows) {
            if (oob) *oob = 1;
            continue;
        }
        // run length, 1 .. 64: the group's lanes compare the next 16 ids at a time (position j + 64 differs or is past the end,
        // so the fourth round at the latest sees a mismatch)
        int r = 1;
        for (;;) {
            const int64_t t = j + r + lig;
            const bool eq = t < n && ids[t] == id;
            const unsigned mask = (unsigned)(__ballot(eq) >> shift) & 0xffffu;
            if (mask != 0xffffu) {
                r += __builtin_ctz(~mask);
                break;
            }
            r += kRowGroup;
        }
        const int64_t pr = id * ld;
        for (int c = lig; c < W; c += kRowGroup) {
            const T pv0 = *reinterpret_cast<const T*>(p + pr + V * c);            // in flight under the gradient rows
            const T mv0 = *reinterpret_cast<const T*>(m + pr + V * c);
            const T vv0 = *reinterpret_cast<const T*>(v + pr + V * c);
            T acc = *reinterpret_cast<const T*>(g + (perm ? perm[j] : j) * ld_g + V * c);
            for (int k0 = 1; k0 < r; k0 += 4) {                                   // 4 independent rows in flight, added in order
                T t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kk = k0 + u < r ? k0 + u : r - 1;                   // clamped, not branched: the loads stay unconditional
                    t[u] = *reinterpret_cast<const T*>(g + (perm ? perm[j + kk] : j + kk) * ld_g + V * c);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = acc + (k0 + u < r ? t[u] : row_zero<T>());
            }
            T pv = pv0, mv = mv0, vv = vv0;
            adam_update_chunk(pv, mv, vv, acc, k);
            *reinterpret_cast<T*>(p + pr + V * c) = pv;
            *reinterpret_cast<T*>(m + pr + V * c) = mv;
            *reinterpret_cast<T*>(v + pr + V * c) = vv;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void adam_rows_long_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                              int64_t ld, int64_t rows, int E, const int64_t* __restrict__ ids,
                                                              const int64_t* __restrict__ perm, int64_t n, const float* __restrict__ g,
                                                              int64_t ld_g, AdamCoef k, int32_t* oob) {
    constexpr int V = sizeof(T) / 4;
    constexpr int CB = kRowGroup * V;                     // columns of one pass: 64 floats (16-byte path) or 16
    __shared__ __attribute__((aligned(16))) float part[kLongGroups][CB];
    __shared__ int64_t s_head[16];
    __shared__ int64_t s_end;
    const int W = E / V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lig = threadIdx.x & (kRowGroup - 1), q = threadIdx.x / kRowGroup;
    // every loop bound and branch below that contains a barrier is uniform over the workgroup
    for (int64_t base = (int64_t)blockIdx.x * 1024; base < n; base += (int64_t)gridDim.x * 1024) {
        const int64_t pos = base + threadIdx.x;
        bool long_head = false;
        if (pos + kLongRun < n) {
            const int64_t id = ids[pos];
            long_head = (pos == 0 || ids[pos - 1] != id) && ids[pos + kLongRun] == id;
        }
        const unsigned long long found = __ballot(long_head);         // at most one bit: two long heads are > 64 positions apart
        if (lane == 0) s_head[wave] = found ? base + 64 * wave + __builtin_ctzll(found) : -1;
        __syncthreads();
        for (int w = 0; w < 16; ++w) {
            const int64_t h = s_head[w];
            if (h < 0) continue;
            const int64_t id = ids[h];
            if (id < 0 || id >= rows) {
                if (oob && threadIdx.x == 0) *oob = 1;
                continue;
            }
            if (wave == 0) {
                // end of the run by a 64-way search: ids[lo - 1] == id, and ids[hi] != id or hi == n; every round the 64 lanes probe
                // evenly spaced positions of [lo, hi) — the equal ones are a prefix — and the span shrinks below the stride
                int64_t lo = h + kLongRun + 1, hi = n;
                while (lo < hi) {
                    const int64_t stride = (hi - lo + 63) / 64;
                    const int64_t t = lo + lane * stride;
                    const unsigned long long eq = __ballot(t < hi && ids[t] == id);
                    const int cnt = ~eq ? __builtin_ctzll(~eq) : 64;
                    if (cnt == 0) {
                        hi = lo;
                    } else {
                        const int64_t next = lo + cnt * stride;
                        lo = lo + (cnt - 1) * stride + 1;
                        if (cnt < 64 && next < hi) hi = next;
                    }
                }
                if (lane == 0) s_end = lo;
            }
            __syncthreads();
            const int64_t r = s_end - h;                              // > 64
            const int64_t pr = id * ld;
            for (int c0 = 0; c0 < W; c0 += kRowGroup) {               // column passes of CB floats
                const bool live = c0 + lig < W;
                const int c = live ? c0 + lig : 0;                    // idle lanes re-read chunk 0 and drop it
                T acc = row_zero<T>();
                for (int64_t k0 = q; k0 < r; k0 += (int64_t)kLongGroups * kLongFlight) {
                    T t[kLongFlight];
#pragma unroll
                    for (int u = 0; u < kLongFlight; ++u) {
                        const int64_t kk = k0 + (int64_t)kLongGroups * u;
                        const int64_t at = h + (kk < r ? kk : r - 1);
                        t[u] = *reinterpret_cast<const T*>(g + (perm ? perm[at] : at) * ld_g + V * c);
                    }
#pragma unroll
                    for (int u = 0; u < kLongFlight; ++u) acc = acc + (k0 + (int64_t)kLongGroups * u < r ? t[u] : row_zero<T>());
                }
                *reinterpret_cast<T*>(&part[q][V * lig]) = acc;
                __syncthreads();
                const int col = V * c0 + threadIdx.x;
                if (threadIdx.x < CB && col < E) {
                    float s = part[0][threadIdx.x];
                    for (int s_q = 1; s_q < kLongGroups; ++s_q) s += part[s_q][threadIdx.x];
                    float pj = p[pr + col], mj = m[pr + col], vj = v[pr + col];
                    adam_update(pj, mj, vj, s, k);
                    p[pr + col] = pj;
                    m[pr + col] = mj;
                    v[pr + col] = vj;
                }
                __syncthreads();
            }
        }
        __syncthreads();                                              // s_head is rewritten by the next tile
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_adam_rows(float* p, float* m, float* v, int64_t ld, int64_t rows, int E, const int64_t* sorted_ids, const int64_t* perm,
                             int64_t n, const float* g, int64_t ld_g, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int64_t step, int32_t* oob, ncf_stream_t stream) {
    if (n == 0) return NCF_OK;
    if (n < 0 || rows < 0 || E <= 0 || step < 1 || ld < E || ld_g < E || !p || !m || !v || !sorted_ids || !g)
        return fail(NCF_EINVAL, "ncf_adam_rows: bad argument");
    const AdamCoef k = adam_coef(lr, beta1, beta2, eps, weight_decay, step);
    const bool vec = E % 4 == 0 && ld % 4 == 0 && ld_g % 4 == 0 && aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g);
    hipStream_t s = (hipStream_t)stream;
    int64_t blocks = (n + 256 / kRowGroup - 1) / (256 / kRowGroup);
    if (blocks > 16384) blocks = 16384;
    int64_t long_blocks = (n + 1023) / 1024;
    if (long_blocks > 1024) long_blocks = 1024;
    if (vec) {
        hipLaunchKernelGGL(adam_rows_kernel<f32x4>, dim3((unsigned)blocks), dim3(256), 0, s, p, m, v, ld, rows, E, sorted_ids, perm, n, g, ld_g, k, oob);
        if (n > kLongRun)
            hipLaunchKernelGGL(adam_rows_long_kernel<f32x4>, dim3((unsigned)long_blocks), dim3(1024), 0, s, p, m, v, ld, rows, E, sorted_ids, perm,
                               n, g, ld_g, k, oob);
    } else {
        hipLaunchKernelGGL(adam_rows_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, p, m, v, ld, rows, E, sorted_ids, perm, n, g, ld_g, k, oob);
        if (n > kLongRun)
            hipLaunchKernelGGL(adam_rows_long_kernel<float>, dim3((unsigned)long_blocks), dim3(1024), 0, s, p, m, v, ld, rows, E, sorted_ids, perm,
                               n, g, ld_g, k, oob);
    }
    return check_launch("ncf_adam_rows");
}
