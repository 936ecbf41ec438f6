// Negative sampling for pair-wise (BPR) training: the per-sample draw of the reference's RankingDataset.__getitem__
// (datasets/base.py:57-78: probs = r ** w / sum(r ** w) over the row's negatives, then np.random.choice) on the device.
//
// The negatives are one CSR with a row per training sample (rowptr int64, item positions int32, ratings fp32).
//   ncf_negative_cdf      once per value of w: each row's normalised inclusive prefix of its weights, written over a buffer
//                         of the same length.  One wave owns one row and streams it three times: (1) the weights themselves
//                         go to the output buffer with their largest value and fp32 sum; (2) each weight is quantised to
//                         64-bit fixed point relative to the row's largest one and the integers summed; (3) an integer wave
//                         scan with a running carry gives each prefix, divided by the total in double and rounded to fp32.
//                         Integer sums are exact, so the prefix does not depend on the scan's order: it is non-decreasing,
//                         a zero weight repeats its predecessor's value bit for bit (it can never be drawn), and the last
//                         entry is total / total = 1.0f exactly.  A row of at most 512 entries keeps its weights in registers
//                         (one load round trip per row); a longer one is streamed, passes 2 and 3 re-reading what pass 1 wrote,
//                         from L2.  Both forms quantise and scan in the same order: the same bits.
//   ncf_sample_negatives  one lane per sample: u from a counter-based hash of (seed, slot), then an upper-bound binary
//                         search over the row's CDF (the number of entries <= u, numpy's searchsorted side='right').
// No atomics: the same inputs give the same bits.
#include "ncf_common.h"
#include <math.h>

namespace ncf {
namespace {

constexpr int kCdfUnroll = 8;   // pass 1 keeps 8 independent 256-byte wave loads in flight; rows of <= 512 entries stay in registers

// include/ncf_abi.h states this formula; tests restate it in numpy
__device__ __forceinline__ float slot_uniform(uint32_t seed, uint64_t slot) {
    return (float)(slot_hash(seed, slot) >> 8) * 0x1p-24f;   // 24 bits: exact in fp32, in [0, 1)
}

__device__ __forceinline__ float neg_weight(float r, float w) { return w == 0.f ? 1.f : powf(r, w); }   // numpy: 0 ** 0 == 1

__device__ __forceinline__ int64_t quantise(float wt, double scale) {   // a positive weight keeps a non-zero share
    if (!(wt > 0.f)) return 0;
    const double q = rint((double)wt * scale);
    return q < 1.0 ? 1 : (int64_t)q;
}

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) {
    const int lo = __shfl_up((int)(uint32_t)v, d), hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), d);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// one 64-entry chunk of pass 3: inclusive integer scan, (carry + prefix) / total written where the lane holds an entry; the new carry
__device__ __forceinline__ int64_t scan_chunk(int64_t q, int lane, bool live, int64_t carry, double dtot, float* out) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = shfl_up64(q, d);
        if (lane >= d) q += t;
    }
    if (live) *out = (float)((double)(carry + q) / dtot);
    return carry + shfl64(q, 63);
}

__global__ __launch_bounds__(256) void negative_cdf_kernel(const int64_t* __restrict__ rowptr, int64_t rows,
                                                           const float* __restrict__ rating, float w, float* __restrict__ cdf,
                                                           int32_t* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const int64_t beg = rowptr[r], end = rowptr[r + 1];
        const int64_t len = end - beg;
        // pass 1: weights, their largest value and fp32 sum (a NaN or an overflow shows in the sum)
        const bool in_regs = len <= 64 * kCdfUnroll;   // wave-uniform
        float wreg[kCdfUnroll];
        float mx = 0.f, s = 0.f;
        for (int64_t k0 = beg; k0 < end; k0 += 64 * kCdfUnroll) {
            float rv[kCdfUnroll];
#pragma unroll
            for (int u = 0; u < kCdfUnroll; ++u) {
                const int64_t k = k0 + u * 64 + lane;
                rv[u] = k < end ? rating[k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kCdfUnroll; ++u) {
                const int64_t k = k0 + u * 64 + lane;
                wreg[u] = 0.f;
                if (k < end) {
                    const float wt = neg_weight(rv[u], w);
                    wreg[u] = wt;
                    if (!in_regs) cdf[k] = wt;
                    mx = fmaxf(mx, wt);
                    s += wt;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {   // butterfly: every lane ends with the same bits
            mx = fmaxf(mx, __shfl_xor(mx, off));
            s += __shfl_xor(s, off);
        }
        if (!(isfinite(s) && s > 0.f)) {   // no distribution: flag it, and leave a uniform CDF that a draw can still read
            if (lane == 0) *flag = 1;
            for (int64_t k = beg + lane; k < end; k += 64) cdf[k] = (float)((double)(k - beg + 1) / (double)len);
            continue;
        }
        // pass 2: fixed point with S fractional bits against the largest weight; len * 2^S < 2^62 keeps every sum in int64
        const int S = 62 - (64 - __clzll((unsigned long long)len));
        const double scale = ldexp(1.0, S) / (double)mx;
        int64_t tot = 0;
        if (in_regs) {
#pragma unroll
            for (int u = 0; u < kCdfUnroll; ++u)
                if (beg + u * 64 + lane < end) tot += quantise(wreg[u], scale);
        } else {
            for (int64_t k = beg + lane; k < end; k += 64) tot += quantise(cdf[k], scale);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tot += shfl_xor64(tot, off);
        // pass 3: inclusive scan, chunk by chunk, each prefix over the total
        const double dtot = (double)tot;
        int64_t carry = 0;
        if (in_regs) {
#pragma unroll
            for (int u = 0; u < kCdfUnroll; ++u) {
                if (beg + u * 64 < end) {   // wave-uniform
                    const int64_t k = beg + u * 64 + lane;
                    carry = scan_chunk(k < end ? quantise(wreg[u], scale) : 0, lane, k < end, carry, dtot, cdf + k);
                }
            }
        } else {
            for (int64_t k0 = beg; k0 < end; k0 += 64) {
                const int64_t k = k0 + lane;
                carry = scan_chunk(k < end ? quantise(cdf[k], scale) : 0, lane, k < end, carry, dtot, cdf + k);
            }
        }
    }
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(const int64_t* __restrict__ rowptr, const float* __restrict__ cdf,
                                                               const int32_t* __restrict__ neg, int64_t rows,
                                                               const int64_t* __restrict__ pick, int64_t n, uint32_t seed,
                                                               int64_t slot0, int64_t* __restrict__ out, int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n; b += stride) {
        const int64_t r = pick[b];
        int64_t res = -1;
        bool ok = false;
        if (r >= 0 && r < rows) {
            const int64_t beg = rowptr[r], len = rowptr[r + 1] - beg;
            if (len > 0) {
                const float u = slot_uniform(seed, (uint64_t)(slot0 + b));
                int64_t lo = 0, hi = len;   // upper bound: entries <= u
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (cdf[beg + mid] <= u) lo = mid + 1;
                    else hi = mid;
                }
                res = neg[beg + (lo < len ? lo : len - 1)];   // lo == len only where the row's CDF does not end in 1
                ok = true;
            }
        }
        if (!ok && flag) *flag = 1;
        out[b] = res;
    }
}

}  // namespace
}  // namespace ncf

using namespace ncf;

extern "C" int ncf_negative_cdf(const int64_t* rowptr, int64_t rows, const float* rating, float w, float* cdf, int32_t* flag,
                                ncf_stream_t stream) {
    if (rows < 0 || !(w >= 0.f)) return fail(NCF_EINVAL, "ncf_negative_cdf: bad argument (rows %lld, w %g)", (long long)rows, (double)w);
    if (!rowptr || !rating || !cdf || !flag) return fail(NCF_EINVAL, "ncf_negative_cdf: null pointer");
    if (rows == 0) return NCF_OK;
    int64_t blocks = (rows + 3) / 4;
    const int64_t cap = (int64_t)num_cus() * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(negative_cdf_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, rows, rating, w, cdf, flag);
    return check_launch("ncf_negative_cdf");
}

extern "C" int ncf_sample_negatives(const int64_t* rowptr, const float* cdf, const int32_t* neg, int64_t rows, const int64_t* pick,
                                    int64_t n, uint32_t seed, int64_t slot0, int64_t* out, int32_t* flag, ncf_stream_t stream) {
    if (rows < 0 || n < 0 || slot0 < 0) return fail(NCF_EINVAL, "ncf_sample_negatives: bad argument (rows %lld, n %lld, slot0 %lld)",
                                                    (long long)rows, (long long)n, (long long)slot0);
    if (!rowptr || !cdf || !neg) return fail(NCF_EINVAL, "ncf_sample_negatives: null pointer");
    if (n == 0) return NCF_OK;
    if (!pick || !out) return fail(NCF_EINVAL, "ncf_sample_negatives: null pointer");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, cdf, neg, rows, pick, n,
                       seed, slot0, out, flag);
    return check_launch("ncf_sample_negatives");
}
