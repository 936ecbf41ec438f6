// Fixed user profiles of the content form of BasicNCF (FixedProfilesProvider) and of the content-based baseline, for gfx950:
//     out[u, f] = (float)( sum over the ratings e of user u, in order, of ((double)rating[e] - avg[u]) * (double)features[col[e], f]  /  n_u )
// the reference's create_user_embedding (create_dataset.ipynb), one user at a time in a Python loop there.
//
// One wave owns one (user, 256-column chunk) and walks the user's row of the CSR from its first entry to its last: a row is never
// split over waves, there are no atomics and no cross-lane reduction, so the double-precision sum of every column runs in the
// order of the contract and the result is a fixed function of the inputs.  Lanes run across columns: 16-byte loads, 4 consecutive
// columns per lane, where F, the leading dimensions and the base addresses allow; else one column per lane, four times (columns
// lane, lane + 64, ...).
//
// The row's entries come in blocks of 64: lane l fetches col / rating of entry l of the block (one coalesced load each, the next
// block's requested before this one is used) and computes rating - avg in double; every entry is then handed to the whole wave as
// a UNIFORM value (v_readlane into scalar registers), so the branches on it are scalar branches and a feature row's address is a
// scalar base plus the lane's column.  Inside a block, NCF_UP_ROWS feature rows are requested at a time, the next group before the
// current one is added, and added strictly in row order.  (Plain uniform loads of col / rating are not an option here: the kernel
// stores to memory, so the compiler cannot prove them invariant and turns them into per-lane loads with a wait after each.)
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py EXTRA_FLAGS): the contract rounds the product and then the sum, which a
// fused multiply-add would not.  The pragma below says the same to a build that forgets the flag.
//
// Bytes: 4 * F per rating from the feature table (which the Infinity Cache holds at the reference's size: a few thousand items of
// F ~ 1200), 8 per rating and 256-column chunk of col + rating, 4 * F per user written.
#include "ncf_common.h"

#pragma clang fp contract(off)

#ifndef NCF_UP_ROWS
#define NCF_UP_ROWS 8          // feature rows per group: two groups are in flight per wave.  64 % NCF_UP_ROWS == 0
#endif
#define NCF_UP_CHUNK 256       // columns per wave
#define NCF_UP_MAXBLOCKS (1 << 20)

namespace ncf {

// VEC: lane l holds columns c0 + 4 l .. c0 + 4 l + 3 (one 16-byte load per row); else columns c0 + l + 64 j, j < 4.
template <bool VEC>
__global__ __launch_bounds__(256) void user_profiles_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ rating, int64_t nnz,
    const double* __restrict__ avg, int64_t U, const float* __restrict__ feat, int64_t I, int64_t ldf, int F, int nchunks,
    float* __restrict__ out, int64_t ldout, int32_t* oob) {
    constexpr int R = NCF_UP_ROWS;
    static_assert(64 % R == 0, "a block of 64 entries is whole groups");
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t total = U * nchunks;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < total; w += nwaves) {
        const int64_t u = w / nchunks;
        const int c0 = (int)(w - u * nchunks) * NCF_UP_CHUNK;
        int64_t beg = uniform64(rowptr[u]), end = uniform64(rowptr[u + 1]);
        if (beg < 0 || end > nnz || end < beg) {           // a row pointer outside the arrays: nothing of it is read
            if (oob && lane == 0) *oob = 1;
            beg = end = 0;
        }
        const double a = avg[u];
        int cidx[4];
        bool live[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cidx[j] = VEC ? c0 + 4 * lane + j : c0 + lane + 64 * j;
            live[j] = cidx[j] < F;
        }
        // one group's feature rows: entry g + r of the block, wherever its column is inside the table
        auto load_group = [&](int cv, int g, float (&v)[R][4]) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int c = __builtin_amdgcn_readlane(cv, g + r);
                if (c >= 0 && (int64_t)c < I) {
                    const float* row = feat + (int64_t)c * ldf;
                    if (VEC) {
                        if (live[0]) {                     // F % 4 == 0: a lane's four columns are inside the row together
                            const f32x4 q = *reinterpret_cast<const f32x4*>(row + cidx[0]);
                            v[r][0] = q.x; v[r][1] = q.y; v[r][2] = q.z; v[r][3] = q.w;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (live[j]) v[r][j] = row[cidx[j]];
                    }
                }
            }
        };
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int cv_next = -1;                                  // -1: no entry (past the row's end) — out of every table's range
        float rv_next = 0.f;
        if (beg + lane < end) {
            cv_next = col[beg + lane];
            rv_next = rating[beg + lane];
        }
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            const int cv = cv_next;
            const double dv = (double)rv_next - a;
            const int nb = (int)(end - e0 < 64 ? end - e0 : 64);
            cv_next = -1;
            rv_next = 0.f;
            if (e0 + 64 + lane < end) {                    // the next block's entries, requested before this block is used
                cv_next = col[e0 + 64 + lane];
                rv_next = rating[e0 + 64 + lane];
            }
            if (lane < nb && !(cv >= 0 && (int64_t)cv < I) && oob) *oob = 1;
            const int dlo = __double2loint(dv), dhi = __double2hiint(dv);
            float cur[R][4] = {}, nxt[R][4] = {};
            load_group(cv, 0, cur);
            for (int g = 0; g < nb; g += R) {              // g + r <= 63: nb <= 64 and R divides 64
                if (g + R < nb) load_group(cv, g + R, nxt);
#pragma unroll
                for (int r = 0; r < R; ++r) {              // in row order; an entry past the row or out of range adds nothing
                    const int c = __builtin_amdgcn_readlane(cv, g + r);
                    if (c >= 0 && (int64_t)c < I) {
                        const double d = __hiloint2double(__builtin_amdgcn_readlane(dhi, g + r), __builtin_amdgcn_readlane(dlo, g + r));
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double p = d * (double)cur[r][j];
                            acc[j] = acc[j] + p;
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) cur[r][j] = nxt[r][j];
            }
        }
        const int64_t n = end - beg;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = n > 0 ? (float)(acc[j] / (double)n) : 0.f;
        float* orow = out + u * ldout;
        if (VEC) {
            if (live[0]) *reinterpret_cast<f32x4*>(orow + cidx[0]) = f32x4{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j]) orow[cidx[j]] = o[j];
        }
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_user_profiles(const int64_t* rowptr, const int32_t* col, const float* rating, int64_t nnz, const double* avg, int64_t U,
                                 const float* features, int64_t I, int64_t ldf, int F, float* out, int64_t ldout, int32_t* oob,
                                 ncf_stream_t stream) {
    if (U < 0 || I < 0 || nnz < 0) return fail(NCF_EINVAL, "ncf_user_profiles: negative size U=%lld I=%lld nnz=%lld", (long long)U, (long long)I, (long long)nnz);
    if (F <= 0) return fail(NCF_EINVAL, "ncf_user_profiles: F = %d", F);
    if (ldf < F || ldout < F) return fail(NCF_EINVAL, "ncf_user_profiles: leading dimension smaller than row (F=%d ldf=%lld ldout=%lld)", F, (long long)ldf, (long long)ldout);
    if (U == 0) return NCF_OK;
    if (!rowptr || !avg || !out) return fail(NCF_EINVAL, "ncf_user_profiles: null pointer");
    if (nnz > 0 && (!col || !rating)) return fail(NCF_EINVAL, "ncf_user_profiles: %lld entries without col / rating", (long long)nnz);
    if (nnz > 0 && I > 0 && !features) return fail(NCF_EINVAL, "ncf_user_profiles: null feature table");
    const int nchunks = (F + NCF_UP_CHUNK - 1) / NCF_UP_CHUNK;
    const int64_t waves = U * nchunks;
    int64_t blocks = (waves + 3) / 4;
    if (blocks > NCF_UP_MAXBLOCKS) blocks = NCF_UP_MAXBLOCKS;     // grid-stride beyond
    const bool vec = F % 4 == 0 && ldf % 4 == 0 && ldout % 4 == 0 && aligned16(features) && aligned16(out);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(user_profiles_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, rating, nnz, avg, U, features, I,
                           ldf, F, nchunks, out, ldout, oob);
    else
        hipLaunchKernelGGL(user_profiles_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, rating, nnz, avg, U, features, I,
                           ldf, F, nchunks, out, ldout, oob);
    return check_launch("ncf_user_profiles");
}
