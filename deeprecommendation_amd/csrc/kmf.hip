// KernelMF, the collaborative-filtering baseline of the reference's evaluation (cf_baseline.py: the matrix_factorization package's
// biased MF with the linear kernel), fitted by stratified SGD on gfx950:
//     r^ = mu + b_u + b_i + p_u . q_i,     one SGD update per rating, in a fixed order.
//
// Per-sample SGD is a serial chain: an update reads what the one before it wrote.  The rating matrix is cut into W x W blocks
// (DSGD, Gemulla et al. 2011); stratum s holds the blocks (a, (a + s) mod W), a = 0 .. W-1, which share no user row and no item row,
// so the W chains of a stratum run side by side and give the bits of any sequential order of those blocks.  One launch is one
// stratum: W workgroups of ONE wave, wave a walks block (s, a) from its first sample to its last.  The hand-off from one stratum to
// the next is the launch boundary and nothing else: no grid barrier, no flag, no atomics on floats.
//
// Table rows are (F factors, bias, padding).  A wave spreads a row over its lanes, 4 consecutive columns per lane (F <= 256: column c
// is lane c / 4), one 16-byte access per lane and row where the leading dimension and the base address allow and single floats
// otherwise (and always for a lane whose four columns are not all factors).  The bias, column F, is read and written by the lane that
// owns column F and handed to the others with v_readlane.  Columns beyond F are never touched.  Both tables are MODIFIED by the kernel
// that reads them, so they are plain (non-const, non-restrict) pointers and every access to them is a vector load or store.
//
// The samples come in groups of 64: lane l fetches sample l of the group (coalesced) and CHECKS it — ids inside the tables, the
// user's and the item's block the ones of this wave — before anything is dereferenced through it; a ballot then says which samples
// the wave walks, each handed to all lanes as a uniform value.
//
// THIS FILE IS BUILT WITH -ffp-contract=off (build.py EXTRA_FLAGS): every product and every sum of the contract (include/ncf_abi.h)
// is rounded on its own.  The pragma below says the same to a build that forgets the flag.
#include "ncf_common.h"

#include <math.h>

#pragma clang fp contract(off)

#define NCF_KMF_MAX_F 256
#define NCF_KMF_MAX_W 1024
#define NCF_KMF_FOLD_MAXBLOCKS (1 << 16)

namespace ncf {

__device__ __forceinline__ float kmf_lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// the lane's nc (0 .. 4) factor columns c0 .. c0 + nc - 1 of one row
template <bool VEC>
__device__ __forceinline__ void kmf_load(const float* row, int c0, int nc, float (&v)[4]) {
    if (VEC && nc == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(row + c0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nc) v[j] = row[c0 + j];
    }
}

template <bool VEC>
__device__ __forceinline__ void kmf_store(float* row, int c0, int nc, const float (&v)[4]) {
    if (VEC && nc == 4) {
        *reinterpret_cast<f32x4*>(row + c0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nc) row[c0 + j] = v[j];
    }
}

// dot of the contract: the lane's partial sum in column order, then the balanced tree over the lanes.  An xor butterfly gives the
// tree's value in every lane: each level adds the sums of two neighbouring groups, and a + b == b + a in fp32.
__device__ __forceinline__ float kmf_dot(const float (&p)[4], const float (&q)[4], int nc) {
    float part = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nc) {
            const float t = p[j] * q[j];
            part = part + t;
        }
    part = part + __shfl_xor(part, 1);
    part = part + __shfl_xor(part, 2);
    part = part + __shfl_xor(part, 4);
    part = part + __shfl_xor(part, 8);
    part = part + __shfl_xor(part, 16);
    part = part + __shfl_xor(part, 32);
    return part;
}

// x - lr * (err * y + reg * x)
__device__ __forceinline__ float kmf_step(float x, float y, float err, float lr, float reg) {
    const float g = err * y;
    const float d = reg * x;
    const float t = g + d;
    const float m = lr * t;
    return x - m;
}

// b - lr * (err + reg * b)
__device__ __forceinline__ float kmf_bias_step(float b, float err, float lr, float reg) {
    const float d = reg * b;
    const float t = err + d;
    const float m = lr * t;
    return b - m;
}

// One stratum: wave a = blockIdx.x walks block (s, a).
template <bool VEC>
__global__ __launch_bounds__(64) void kmf_stratum_kernel(
    float* PU, int64_t ldu, int64_t U, float* QI, int64_t ldq, int64_t I, int F, const int32_t* __restrict__ user,
    const int32_t* __restrict__ item, const float* __restrict__ rating, int64_t n, const int64_t* __restrict__ block_ptr,
    const int32_t* __restrict__ user_block, const int32_t* __restrict__ item_block, int W, int s, float mu, float lr, float reg,
    double* sse_row, int32_t* flag) {
    const int lane = threadIdx.x;
    const int a = blockIdx.x;
    const int ib = a + s >= W ? a + s - W : a + s;
    const int64_t slot = (int64_t)s * W + a;
    int64_t beg = uniform64(block_ptr[slot]), end = uniform64(block_ptr[slot + 1]);
    if (beg < 0 || end > n || end < beg) {                 // a block pointer outside the samples: nothing of the block is read
        if (flag && lane == 0) atomicOr(flag, NCF_KMF_FLAG_PTR);
        beg = end = 0;
    }
    const int c0 = 4 * lane;
    const int nc = F - c0 >= 4 ? 4 : F - c0 > 0 ? F - c0 : 0;
    const int bl = (F >> 2) & 63;                          // the lane that owns column F
    double sse = 0.0;
    for (int64_t e0 = beg; e0 < end; e0 += 64) {
        const int nb = (int)(end - e0 < 64 ? end - e0 : 64);
        int uv = -1, iv = -1;
        float rv = 0.f;
        bool ok = false;
        if (lane < nb) {
            uv = user[e0 + lane];
            iv = item[e0 + lane];
            rv = rating[e0 + lane];
            if (!(uv >= 0 && (int64_t)uv < U && iv >= 0 && (int64_t)iv < I)) {
                if (flag) atomicOr(flag, NCF_KMF_FLAG_ID);
            } else if (user_block[uv] != a || item_block[iv] != ib) {
                if (flag) atomicOr(flag, NCF_KMF_FLAG_BLOCK);
            } else {
                ok = true;
            }
        }
        const uint64_t live = __ballot(ok);
        for (int g = 0; g < nb; ++g) {
            if (!((live >> g) & 1)) continue;              // a flagged sample writes nothing
            const int u = __builtin_amdgcn_readlane(uv, g);
            const int i = __builtin_amdgcn_readlane(iv, g);
            const float r = kmf_lane_value(rv, g);
            float* prow = PU + (int64_t)u * ldu;
            float* qrow = QI + (int64_t)i * ldq;
            float p[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
            float bu = 0.f, bi = 0.f;
            kmf_load<VEC>(prow, c0, nc, p);
            kmf_load<VEC>(qrow, c0, nc, q);
            if (lane == bl) {
                bu = prow[F];
                bi = qrow[F];
            }
            bu = kmf_lane_value(bu, bl);
            bi = kmf_lane_value(bi, bl);
            const float dot = kmf_dot(p, q, nc);
            const float base = mu + bi;
            const float both = base + bu;
            const float pred = both + dot;
            const float err = pred - r;
            if (lane == bl) {
                prow[F] = kmf_bias_step(bu, err, lr, reg);
                qrow[F] = kmf_bias_step(bi, err, lr, reg);
            }
            float pn[4], qn[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pn[j] = kmf_step(p[j], q[j], err, lr, reg);
                qn[j] = kmf_step(q[j], p[j], err, lr, reg);
            }
            kmf_store<VEC>(prow, c0, nc, pn);
            kmf_store<VEC>(qrow, c0, nc, qn);
            const double de = (double)err;
            sse = sse + de * de;
        }
    }
    if (sse_row && lane == 0) sse_row[a] = sse_row[a] + sse;   // the only writer of this word while the launch runs
}

// Fold-in: wave k fits the row of user users[k] against the fixed item table; the row stays in registers over all passes.
template <bool VEC>
__global__ __launch_bounds__(64) void kmf_fold_kernel(
    float* PU, int64_t ldu, int64_t U, const float* __restrict__ QI, int64_t ldq, int64_t I, int F, const int32_t* __restrict__ users,
    int64_t n_users, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ rating, int64_t nnz,
    float mu, float lr, float reg, int n_epochs, double* sse_out, int32_t* flag) {
    const int lane = threadIdx.x;
    const int c0 = 4 * lane;
    const int nc = F - c0 >= 4 ? 4 : F - c0 > 0 ? F - c0 : 0;
    const int bl = (F >> 2) & 63;
    for (int64_t k = blockIdx.x; k < n_users; k += gridDim.x) {
        const int u = __builtin_amdgcn_readfirstlane(users[k]);
        if (!(u >= 0 && (int64_t)u < U)) {                 // nothing is read or written through this id
            if (flag && lane == 0) atomicOr(flag, NCF_KMF_FLAG_ID);
            continue;
        }
        int64_t beg = uniform64(rowptr[k]), end = uniform64(rowptr[k + 1]);
        if (beg < 0 || end > nnz || end < beg) {
            if (flag && lane == 0) atomicOr(flag, NCF_KMF_FLAG_PTR);
            beg = end = 0;
        }
        float* prow = PU + (int64_t)u * ldu;
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        float bu = 0.f;
        kmf_load<VEC>(prow, c0, nc, p);
        if (lane == bl) bu = prow[F];
        bu = kmf_lane_value(bu, bl);
        for (int ep = 0; ep < n_epochs; ++ep) {
            double sse = 0.0;
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                const int nb = (int)(end - e0 < 64 ? end - e0 : 64);
                int iv = -1;
                float rv = 0.f;
                bool ok = false;
                if (lane < nb) {
                    iv = col[e0 + lane];
                    rv = rating[e0 + lane];
                    ok = iv >= 0 && (int64_t)iv < I;
                    if (!ok && flag) atomicOr(flag, NCF_KMF_FLAG_ID);
                }
                const uint64_t live = __ballot(ok);
                for (int g = 0; g < nb; ++g) {
                    if (!((live >> g) & 1)) continue;
                    const int i = __builtin_amdgcn_readlane(iv, g);
                    const float r = kmf_lane_value(rv, g);
                    const float* qrow = QI + (int64_t)i * ldq;
                    float q[4] = {0.f, 0.f, 0.f, 0.f};
                    float bi = 0.f;
                    kmf_load<VEC>(qrow, c0, nc, q);
                    if (lane == bl) bi = qrow[F];
                    bi = kmf_lane_value(bi, bl);
                    const float dot = kmf_dot(p, q, nc);
                    const float base = mu + bi;
                    const float both = base + bu;
                    const float pred = both + dot;
                    const float err = pred - r;
                    bu = kmf_bias_step(bu, err, lr, reg);
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[j] = kmf_step(p[j], q[j], err, lr, reg);
                    const double de = (double)err;
                    sse = sse + de * de;
                }
            }
            if (sse_out && lane == 0) sse_out[(int64_t)ep * n_users + k] = sse;
        }
        kmf_store<VEC>(prow, c0, nc, p);
        if (lane == bl) prow[F] = bu;
    }
}

static int kmf_check_tables(const char* who, int64_t ldu, int64_t U, int64_t ldq, int64_t I, int F, float lr, float reg, int n_epochs) {
    if (U < 0 || I < 0 || n_epochs < 0) return fail(NCF_EINVAL, "%s: negative size U=%lld I=%lld n_epochs=%d", who, (long long)U, (long long)I, n_epochs);
    if (F <= 0) return fail(NCF_EINVAL, "%s: F = %d", who, F);
    if (F > NCF_KMF_MAX_F) return fail(NCF_EUNSUPPORTED, "%s: F = %d factors (at most %d)", who, F, NCF_KMF_MAX_F);
    if (ldu < (int64_t)F + 1 || ldq < (int64_t)F + 1)
        return fail(NCF_EINVAL, "%s: a row holds F + 1 = %d floats (ldu=%lld ldq=%lld)", who, F + 1, (long long)ldu, (long long)ldq);
    if (!isfinite(lr) || !isfinite(reg)) return fail(NCF_EINVAL, "%s: lr / reg not finite", who);
    return NCF_OK;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_kmf_epoch(float* PU, int64_t ldu, int64_t U, float* QI, int64_t ldq, int64_t I, int F, const int32_t* user,
                             const int32_t* item, const float* rating, int64_t n, const int64_t* block_ptr, const int32_t* user_block,
                             const int32_t* item_block, int W, float mu, float lr, float reg, int n_epochs, double* dev_sse,
                             int32_t* dev_flag, ncf_stream_t stream) {
    if (n < 0) return fail(NCF_EINVAL, "ncf_kmf_epoch: negative size n=%lld", (long long)n);
    if (const int rc = kmf_check_tables("ncf_kmf_epoch", ldu, U, ldq, I, F, lr, reg, n_epochs)) return rc;
    if (W < 1 || W > NCF_KMF_MAX_W) return fail(NCF_EINVAL, "ncf_kmf_epoch: W = %d blocks per side (1 .. %d)", W, NCF_KMF_MAX_W);
    if (!PU || !QI || !block_ptr || !user_block || !item_block) return fail(NCF_EINVAL, "ncf_kmf_epoch: null table or plan");
    if (n > 0 && (!user || !item || !rating)) return fail(NCF_EINVAL, "ncf_kmf_epoch: %lld samples without user / item / rating", (long long)n);
    if (n == 0 || n_epochs == 0) return NCF_OK;
    const bool vec = ldu % 4 == 0 && ldq % 4 == 0 && aligned16(PU) && aligned16(QI);
    hipStream_t st = (hipStream_t)stream;
    for (int e = 0; e < n_epochs; ++e) {
        double* sse_row = dev_sse ? dev_sse + (int64_t)e * W : nullptr;
        for (int s = 0; s < W; ++s) {
            if (vec)
                hipLaunchKernelGGL(kmf_stratum_kernel<true>, dim3((unsigned)W), dim3(64), 0, st, PU, ldu, U, QI, ldq, I, F, user, item, rating,
                                   n, block_ptr, user_block, item_block, W, s, mu, lr, reg, sse_row, dev_flag);
            else
                hipLaunchKernelGGL(kmf_stratum_kernel<false>, dim3((unsigned)W), dim3(64), 0, st, PU, ldu, U, QI, ldq, I, F, user, item, rating,
                                   n, block_ptr, user_block, item_block, W, s, mu, lr, reg, sse_row, dev_flag);
        }
        if (const int rc = check_launch("ncf_kmf_epoch")) return rc;
    }
    return NCF_OK;
}

extern "C" int ncf_kmf_fold_users(float* PU, int64_t ldu, int64_t U, const float* QI, int64_t ldq, int64_t I, int F, const int32_t* users,
                                  int64_t n_users, const int64_t* rowptr, const int32_t* col, const float* rating, int64_t nnz, float mu,
                                  float lr, float reg, int n_epochs, double* dev_sse, int32_t* dev_flag, ncf_stream_t stream) {
    if (n_users < 0 || nnz < 0) return fail(NCF_EINVAL, "ncf_kmf_fold_users: negative size n_users=%lld nnz=%lld", (long long)n_users, (long long)nnz);
    if (const int rc = kmf_check_tables("ncf_kmf_fold_users", ldu, U, ldq, I, F, lr, reg, n_epochs)) return rc;
    if (n_users > 0 && (!PU || !users || !rowptr)) return fail(NCF_EINVAL, "ncf_kmf_fold_users: null user table, user list or row pointers");
    if (nnz > 0 && (!QI || !col || !rating)) return fail(NCF_EINVAL, "ncf_kmf_fold_users: %lld entries without item table / col / rating", (long long)nnz);
    if (n_users == 0 || n_epochs == 0) return NCF_OK;
    const bool vec = ldu % 4 == 0 && ldq % 4 == 0 && aligned16(PU) && aligned16(QI);
    const unsigned blocks = (unsigned)(n_users < NCF_KMF_FOLD_MAXBLOCKS ? n_users : NCF_KMF_FOLD_MAXBLOCKS);   // grid-stride beyond
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(kmf_fold_kernel<true>, dim3(blocks), dim3(64), 0, st, PU, ldu, U, QI, ldq, I, F, users, n_users, rowptr, col, rating,
                           nnz, mu, lr, reg, n_epochs, dev_sse, dev_flag);
    else
        hipLaunchKernelGGL(kmf_fold_kernel<false>, dim3(blocks), dim3(64), 0, st, PU, ldu, U, QI, ldq, I, F, users, n_users, rowptr, col, rating,
                           nnz, mu, lr, reg, n_epochs, dev_sse, dev_flag);
    return check_launch("ncf_kmf_fold_users");
}
