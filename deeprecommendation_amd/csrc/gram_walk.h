// The walk that computes one row of the sparse Gram matrix X^T X of a (U, I) rating matrix, shared by knn.hip (cosine epilogue) and
// ease.hip (the Gram row itself).  A file that includes this is built with -ffp-contract=off: every product and sum is rounded on
// its own.
#pragma once
#include "ncf_common.h"

#pragma clang fp contract(off)

#define NCF_GRAM_SCAN_MAX 128             // a row of at most this many entries is walked whole (two steps); a longer one from a binary search

namespace ncf {

// [beg, end) of row r of a CSR with nnz entries; an empty range and the out-of-range flag for a pair outside the entries
__device__ __forceinline__ void csr_range(const int64_t* __restrict__ ptr, int64_t r, int64_t nnz, int32_t* oob, int64_t& beg, int64_t& end) {
    beg = ptr[r];
    end = ptr[r + 1];
    if (beg < 0 || end > nnz || end < beg) {
        if (oob) atomicOr(oob, 1);
        beg = end = 0;
    }
}

// One wave, one (item i, tile of columns [t0, t1)): dot[j - t0] = sum over the users u of column i in ascending order of
// v_ui * v_uj, from +0.0f, and with kCount co[j - t0] = the number of those users; both live in LDS.  The wave walks the users of
// column i (the transposed CSR), and for each user its lanes stride over the user's row (the user CSR).  A user holds an item at most
// once, so the lanes of one user never meet; a workgroup barrier between two users orders one user's LDS writes before the next
// user's reads.  Every id is checked before it is used as an address: a user, a column or a pointer outside its array sets *oob and
// adds nothing; tile 0 checks that every walked row ascends strictly and sets *order where one does not.  Ends on a barrier.
template <bool kCount>
__device__ __forceinline__ void gram_row_walk(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const float* __restrict__ val, int64_t nnz, int64_t U, const int64_t* __restrict__ colptr,
                                              const int32_t* __restrict__ row, const float* __restrict__ tval, int64_t nnzT, int64_t I,
                                              int64_t i, int tile, int64_t t0, int64_t t1, float* dot, int* co, int32_t* oob,
                                              int32_t* order) {
    const int lane = threadIdx.x;
    const int tl = (int)(t1 - t0);
    for (int j = lane; j < tl; j += 64) {
        dot[j] = 0.0f;
        if (kCount) co[j] = 0;
    }
    __syncthreads();
    int64_t cb, ce;
    csr_range(colptr, i, nnzT, lane == 0 ? oob : nullptr, cb, ce);
    cb = uniform64(cb);
    ce = uniform64(ce);
    for (int64_t p0 = cb; p0 < ce; p0 += 64) {
        const int nb = (int)(ce - p0 < 64 ? ce - p0 : 64);
        int uv = -1;
        float wv = 0.f;
        bool ok = false;
        if (lane < nb) {
            uv = row[p0 + lane];
            wv = tval[p0 + lane];
            ok = uv >= 0 && (int64_t)uv < U;
            if (!ok && oob) atomicOr(oob, 1);
        }
        const uint64_t live = __ballot(ok);
        for (int g = 0; g < nb; ++g) {
            if (!((live >> g) & 1)) continue;              // nothing is read through a flagged user
            const int u = __builtin_amdgcn_readlane(uv, g);
            const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), g));
            int64_t rb, re;
            csr_range(rowptr, u, nnz, lane == 0 ? oob : nullptr, rb, re);
            rb = uniform64(rb);
            re = uniform64(re);
            const bool whole = tile == 0 || re - rb <= NCF_GRAM_SCAN_MAX;  // tile 0 walks every row whole: it holds the order check
            int64_t e0 = rb;
            if (!whole) {                                  // the first entry with col >= t0 (indices stay inside [rb, re) whatever the row holds)
                int64_t lo = rb, hi = re;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)col[mid] < t0) lo = mid + 1; else hi = mid;
                }
                e0 = uniform64(lo);
            }
            for (; e0 < re; e0 += 64) {
                const int64_t e = e0 + lane;
                bool past = false;
                if (e < re) {
                    const int c = col[e];
                    if (tile == 0 && e > rb && col[e - 1] >= c && order) atomicOr(order, 1);
                    if (c < 0 || (int64_t)c >= I) {
                        if (oob) atomicOr(oob, 1);
                    } else if ((int64_t)c >= t0 && (int64_t)c < t1) {
                        const int j = (int)((int64_t)c - t0);
                        const float t = w * val[e];
                        dot[j] = dot[j] + t;
                        if (kCount) co[j] = co[j] + 1;
                    }
                    past = (int64_t)c >= t1;
                }
                if (!whole && __ballot(past)) break;       // an ascending row has nothing of this tile further on
            }
            __syncthreads();                               // this user's LDS writes before the next user's reads
        }
    }
}

}  // namespace ncf
