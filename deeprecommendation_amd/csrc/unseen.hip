// Unseen negatives for implicit-feedback training and sampled evaluation (He et al. 2017): K distinct items a user has NOT
// interacted with, uniform over what is left, by unranking — no rejection, no retry, no float arithmetic, no atomics.
//
// The seen items are one CSR over users (rowptr int64, item positions int32, strictly ascending inside a row).  Row b of the
// output belongs to user u = pick[b] and slot s = slot0 + b; with A the user's seen row (length a) and M = n_items - a, draw j
// takes r_j in [0, M - j) from the counter-based hash include/ncf_abi.h states and writes the r_j-th smallest element of
// [0, n_items) \ (A u {earlier draws of the row}).
//
// Both steps of a draw are the same search: the r-th element of the complement of a strictly ascending list c is r + k for the
// smallest k with c[k] - k > r (k = the list's length when there is none), because c[k] - k, the number of complement elements
// below c[k], never decreases.  The row's earlier draws are kept as their sorted RANKS in A's complement, p[0 .. j): step 1 skips
// them (q = r + k1 over p, a rank in A's complement; q then enters p at place k1), step 2 skips A (out = q + k2 over A).
//
// Every loop has a bound known before it starts, whatever the input holds: j <= K, ceil(log2(a + 1)) halvings, at most six
// 64-way rounds.  On a row that does not ascend the searches still end with k2 in [0, a], so the output stays in [0, n_items).
//
//   lane form  (K <= 8)   one lane per row, p in eight registers (every index static), a binary search over A per draw.
//   wave form  (K > 8)    one wave per row, p and the row's results in LDS.  Step 1 and the insertion are one descending pass
//                         over p (each lane tests one entry and moves it up one place when it stays above r: j / 64 rounds);
//                         step 2 is a 64-way search (each lane probes one pivot of A: a <= 64 one round, a <= 4160 two); the
//                         K results leave as coalesced stores.
// A refused row (a pick outside the users; fewer unseen items than K) is written as -1 and sets its byte of the flag word: each
// condition has a byte to itself, so a plain byte store of a constant sets it — no read-modify-write to race.
#include "ncf_common.h"

namespace ncf {
namespace {

constexpr int kLaneK = NCF_UNSEEN_LANE_K;   // the lane form's largest K
constexpr int kWaves = 4;                   // waves (rows in flight) per block of the wave form

__device__ __forceinline__ uint32_t draw_rank(uint32_t x, int j, uint32_t left) {   // r_j in [0, left)
    return __umulhi(mix32(x ^ (uint32_t)(j + 1) * 0xC2B2AE35U), left);
}

__device__ __forceinline__ void set_flag(int32_t* flag, int byte) {
    if (flag) reinterpret_cast<volatile unsigned char*>(flag)[byte] = 1;
}

// the row of pick b: false (and the flag byte set) when it is refused
__device__ __forceinline__ bool row_of(const int64_t* __restrict__ rowptr, int64_t users, int64_t n_items, int64_t u, int K,
                                       int64_t& beg, int64_t& a, int32_t* flag) {
    if (u < 0 || u >= users) {
        set_flag(flag, 0);   // NCF_UNSEEN_FLAG_PICK
        return false;
    }
    beg = rowptr[u];
    a = rowptr[u + 1] - beg;
    if (a < 0 || a > n_items || (int64_t)K > n_items - a) {
        set_flag(flag, 1);   // NCF_UNSEEN_FLAG_FEW
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void unseen_lane_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          int64_t users, int64_t n_items, const int64_t* __restrict__ pick, int64_t n,
                                                          int K, uint32_t seed, int64_t slot0, int64_t* __restrict__ out,
                                                          int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n; b += stride) {
        int64_t* o = out + b * K;
        int64_t beg = 0, a = 0;
        if (!row_of(rowptr, users, n_items, pick[b], K, beg, a, flag)) {
            for (int j = 0; j < K; ++j) o[j] = -1;
            continue;
        }
        const int32_t* A = col + beg;
        const uint32_t M = (uint32_t)(n_items - a), x = slot_hash(seed, (uint64_t)(slot0 + b));
        uint32_t p[kLaneK];
#pragma unroll
        for (int i = 0; i < kLaneK; ++i) p[i] = 0;
        for (int j = 0; j < K; ++j) {
            const uint32_t r = draw_rank(x, j, M - (uint32_t)j);
            int k1 = 0;   // p ascends strictly: the entries with p[i] - i <= r are its first k1
#pragma unroll
            for (int i = 0; i < kLaneK; ++i) k1 += (i < j && p[i] - (uint32_t)i <= r) ? 1 : 0;
            const uint32_t q = r + (uint32_t)k1;
#pragma unroll
            for (int i = kLaneK - 1; i > 0; --i) p[i] = i > k1 ? p[i - 1] : p[i];
#pragma unroll
            for (int i = 0; i < kLaneK; ++i) p[i] = i == k1 ? q : p[i];
            int64_t lo = 0, hi = a;   // the smallest k2 with A[k2] - k2 > q, or a
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)A[mid] - mid > (int64_t)q) hi = mid;
                else lo = mid + 1;
            }
            o[j] = (int64_t)q + lo;
        }
    }
}

__global__ __launch_bounds__(64 * kWaves) void unseen_wave_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                  int64_t users, int64_t n_items, const int64_t* __restrict__ pick,
                                                                  int64_t n, int K, uint32_t seed, int64_t slot0,
                                                                  int64_t* __restrict__ out, int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // volatile: a lane's store of p[i + 1] and another lane's load of it in the round before keep their program order
    volatile uint32_t* p = lds + (size_t)wave * 2 * K;
    volatile uint32_t* res = p + K;
    const int64_t nwaves = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < n; b += nwaves) {
        int64_t* o = out + b * K;
        int64_t beg = 0, a = 0;
        if (!row_of(rowptr, users, n_items, pick[b], K, beg, a, flag)) {   // wave-uniform
            for (int j = lane; j < K; j += 64) o[j] = -1;
            continue;
        }
        beg = uniform64(beg), a = uniform64(a);
        const int32_t* A = col + beg;
        const uint32_t M = (uint32_t)(n_items - a), x = slot_hash(seed, (uint64_t)(slot0 + b));
        for (int j = 0; j < K; ++j) {
            const uint32_t r = draw_rank(x, j, M - (uint32_t)j);
            // step 1 and the insertion, from the top round down: an entry that stays above r moves up one place, into a slot
            // whose old value the round above has already read
            int k1 = 0;
            for (int base = (j - 1) & ~63; base >= 0; base -= 64) {   // j == 0: -64, no round
                const int i = base + lane;
                const bool live = i < j;
                const uint32_t v = live ? p[i] : 0u;
                const bool below = live && v - (uint32_t)i <= r;
                if (live && !below) p[i + 1] = v;   // i + 1 <= j <= K - 1
                k1 += __popcll(__ballot(below));
            }
            const uint32_t q = r + (uint32_t)k1;
            if (lane == 0) p[k1] = q;
            // step 2: the smallest k2 in [lo, hi] with A[k2] - k2 > q (hi: none below it).  A round leaves fewer than
            // ceil((hi - lo) / 64) candidates: 2^31 -> 2^25 -> 2^19 -> 2^13 -> 2^7 -> 1 -> 0, six rounds at the most
            int64_t lo = 0, hi = a;
            for (int round = 0; round < 6 && lo < hi; ++round) {
                const int64_t step = (hi - lo + 63) >> 6;
                int64_t t = lo + (int64_t)(lane + 1) * step - 1;
                if (t > hi - 1) t = hi - 1;
                const unsigned long long above = __ballot((int64_t)A[t] - t > (int64_t)q);
                if (above == 0ull) {
                    lo = hi;
                } else {
                    const int f = __ffsll((long long)above) - 1;   // the first lane whose pivot is above
                    int64_t tf = lo + (int64_t)(f + 1) * step - 1;
                    if (tf > hi - 1) tf = hi - 1;
                    if (f > 0) lo = lo + (int64_t)f * step;        // the pivot of lane f - 1, plus one; below tf where f's is unclamped
                    hi = tf;
                    if (lo > hi) lo = hi;                          // two lanes clamped to one pivot
                }
            }
            if (lane == 0) res[j] = (uint32_t)((int64_t)q + lo);   // < n_items < 2^31
        }
        for (int j = lane; j < K; j += 64) o[j] = (int64_t)res[j];
    }
}

}  // namespace
}  // namespace ncf

using namespace ncf;

extern "C" int ncf_sample_unseen(const int64_t* seen_rowptr, const int32_t* seen_col, int64_t users, int64_t n_items, const int64_t* pick,
                                 int64_t n, int K, uint32_t seed, int64_t slot0, int64_t* out, int32_t* flag, ncf_stream_t stream) {
    if (users < 0 || n < 0 || slot0 < 0 || K < 1 || K > NCF_UNSEEN_MAX_K || n_items < 1 || n_items > 2147483647LL)
        return fail(NCF_EINVAL, "ncf_sample_unseen: bad argument (users %lld, n_items %lld, n %lld, K %d, slot0 %lld)", (long long)users,
                    (long long)n_items, (long long)n, K, (long long)slot0);
    if (!seen_rowptr || !flag || (n > 0 && (!pick || !out))) return fail(NCF_EINVAL, "ncf_sample_unseen: null pointer");
    if (n == 0) return NCF_OK;
    const int64_t cap = (int64_t)num_cus() * 8;
    if (K <= kLaneK) {
        int64_t blocks = (n + 255) / 256;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(unseen_lane_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, seen_rowptr, seen_col, users,
                           n_items, pick, n, K, seed, slot0, out, flag);
    } else {
        int64_t blocks = (n + kWaves - 1) / kWaves;
        if (blocks > cap) blocks = cap;
        const size_t lds_bytes = (size_t)kWaves * 2 * K * sizeof(uint32_t);   // 32 KiB at K = 1024
        hipLaunchKernelGGL(unseen_wave_kernel, dim3((unsigned)blocks), dim3(64 * kWaves), lds_bytes, (hipStream_t)stream, seen_rowptr,
                           seen_col, users, n_items, pick, n, K, seed, slot0, out, flag);
    }
    return check_launch("ncf_sample_unseen");
}
