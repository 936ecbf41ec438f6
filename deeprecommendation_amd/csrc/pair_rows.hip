// Shared-row CSR -> per-pair CSR on the stream, with AttentionNCF's train-only target mask applied on the way (gfx950).
//
// A training batch of AttentionNCF carries one CSR row per USER (SparseRatings.pair_row maps pairs to rows); the per-pair attention
// kernels of the autograd path (ncf_attn_forward / ncf_attn_backward) want one row per PAIR, and in training an entry whose rated
// item IS the candidate must be dropped (models/attention_ncf.py:195-205: isclose of the two ItemEmbeddings rows, all elements).
// With torch ops that is repeat_interleave (which reads the entry count back to the host), three index gathers and two
// (nnz, item_emb) gathers for the isclose.  Here, in the pattern of dense_csr.hip — a count kernel, the caller's cumulative sum,
// a fill kernel — so that the host never learns a size:
//   pair_rows_count   one thread per pair: out_rowptr[b + 1] = length of shared row pair_row[b]
//      (cumulative sum of out_rowptr, in place: torch.cumsum on the stream)
//   pair_rows_fill    one wave per pair: the row's (col, val) copied in order to out_rowptr[b]; with the mask, col = -1 where the
//                     candidate's embedding row is close to the rated item's.  The compare reads nnz x E gathered floats, the volume
//                     of the attention kernel's score phase, and takes that phase's layout (attn.hip): LPA lanes per entry on 16-byte
//                     pieces of the rated row, PR_UNROLL entries per lane group in flight, a shuffle AND across the lane group.
// No atomics: the same inputs give the same bits.  Outputs are sized by the caller (capacity); an entry past it is dropped and flagged.
#include "ncf_common.h"

#ifndef PR_UNROLL
#define PR_UNROLL 4           // entries per lane group in flight (independent col -> row loads), as kAttUnroll in attn.hip
#endif

namespace ncf {
namespace {

// torch.isclose(a, b, rtol, atol) in fp32, every operation rounded on its own (no contraction of the multiply into the add):
//   a == b || (isfinite(a) && isfinite(b) && |a - b| <= atol + |rtol * b|)          (include/ncf_abi.h, ncf_pair_rows_fill)
__device__ __forceinline__ bool close_f32(float a, float b, float atol, float rtol) {
    if (a == b) return true;
    if (!(isfinite(a) && isfinite(b))) return false;
    return fabsf(__fsub_rn(a, b)) <= __fadd_rn(atol, fabsf(__fmul_rn(rtol, b)));
}

__global__ __launch_bounds__(256) void pair_rows_count_kernel(const int64_t* __restrict__ rowptr, int64_t R, const int64_t* __restrict__ pair_row,
                                                              int64_t B, int64_t* __restrict__ out_rowptr, int32_t* __restrict__ oob) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) out_rowptr[0] = 0;
    if (b >= B) return;
    const int64_t r = pair_row[b];
    int64_t n = 0;
    if (r >= 0 && r < R) n = rowptr[r + 1] - rowptr[r];
    else if (oob) *oob = 1;
    out_rowptr[b + 1] = n > 0 ? n : 0;
}

// MASK 0: copy only; 1: 16-byte pieces, LPA lanes per entry; 2: generic (any E / leading dimension), one lane per entry
template <int MASK>
__global__ __launch_bounds__(256) void pair_rows_fill_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             const float* __restrict__ val, int64_t R, const int64_t* __restrict__ pair_row,
                                                             int64_t B, const int64_t* __restrict__ out_rowptr, int32_t* __restrict__ out_col,
                                                             float* __restrict__ out_val, int64_t capacity, const float* __restrict__ cand,
                                                             int64_t ldcand, const float* __restrict__ rated, int64_t ldrated, int64_t I, int E,
                                                             float atol, float rtol, int32_t* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;                                      // wave-uniform
    const int64_t r = pair_row[b];
    if (r < 0 || r >= R) return;                             // an empty row (ncf_pair_rows_count raised the out-of-range flag)
    const int64_t src = rowptr[r], len = rowptr[r + 1] - src, dst = out_rowptr[b];
    auto put = [&](int64_t k, int32_t c, float v) {          // entry k of the pair; nothing is written outside [0, capacity)
        const int64_t o = dst + k;
        if (o >= 0 && o < capacity) { out_col[o] = c; out_val[o] = v; }
        else *flag = 1;
    };
    if (MASK == 0) {
        for (int64_t k = lane; k < len; k += 64) put(k, col[src + k], val[src + k]);
    } else if (MASK == 1) {
        const int chunks = E / 4;
        int LPA = 8;
        while (LPA < chunks) LPA <<= 1;                      // 8, 16, 32, 64 lanes per entry
        const int c = lane % LPA, eg = lane / LPA, EPI = 64 / LPA;
        const bool active = c < chunks;
        f32x4 cv = {0.f, 0.f, 0.f, 0.f};
        if (active) cv = *reinterpret_cast<const f32x4*>(cand + b * ldcand + 4 * c);
        constexpr int U = PR_UNROLL;
        for (int64_t k0 = 0; k0 < len; k0 += (int64_t)EPI * U) {       // wave-uniform trip count: the shuffles stay convergent
            f32x4 rv[U];
            int32_t ci[U];
            bool cmp[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + u * EPI + eg;
                ci[u] = -1;
                cmp[u] = false;
                rv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (k < len) {
                    ci[u] = col[src + k];
                    cmp[u] = ci[u] >= 0 && ci[u] < I;        // a column outside the catalogue is copied, never compared
                    if (cmp[u] && active) rv[u] = *reinterpret_cast<const f32x4*>(rated + (int64_t)ci[u] * ldrated + 4 * c);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = k0 + u * EPI + eg;
                int same = 1;
                if (cmp[u] && active)
                    same = close_f32(cv[0], rv[u][0], atol, rtol) && close_f32(cv[1], rv[u][1], atol, rtol) &&
                           close_f32(cv[2], rv[u][2], atol, rtol) && close_f32(cv[3], rv[u][3], atol, rtol);
                for (int off = 1; off < LPA; off <<= 1) same &= __shfl_xor(same, off);
                if (k < len && c == 0) put(k, cmp[u] && same ? -1 : ci[u], val[src + k]);
            }
        }
    } else {
        const float* cr = cand + b * ldcand;
        for (int64_t k = lane; k < len; k += 64) {
            int32_t ci = col[src + k];
            if (ci >= 0 && ci < I) {
                const float* rr = rated + (int64_t)ci * ldrated;
                bool same = true;
                for (int e = 0; e < E && same; ++e) same = close_f32(cr[e], rr[e], atol, rtol);
                if (same) ci = -1;
            }
            put(k, ci, val[src + k]);
        }
    }
}

}  // namespace
}  // namespace ncf

using namespace ncf;

extern "C" int ncf_pair_rows_count(const int64_t* rowptr, int64_t R, const int64_t* pair_row, int64_t B, int64_t* out_rowptr,
                                   int32_t* oob_flag, ncf_stream_t stream) {
    if (R < 0 || B < 0) return fail(NCF_EINVAL, "ncf_pair_rows_count: bad sizes (R %lld, B %lld)", (long long)R, (long long)B);
    if (!out_rowptr) return fail(NCF_EINVAL, "ncf_pair_rows_count: null pointer");
    if (B > 0 && (!rowptr || !pair_row)) return fail(NCF_EINVAL, "ncf_pair_rows_count: null pointer");
    if (B >= (1ll << 31)) return fail(NCF_EUNSUPPORTED, "ncf_pair_rows_count: more than 2^31 pairs");
    if (B == 0) return NCF_OK;                               // an empty batch launches nothing: out_rowptr[0] is the caller's
    hipLaunchKernelGGL(pair_rows_count_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, R, pair_row, B,
                       out_rowptr, oob_flag);
    return check_launch("ncf_pair_rows_count");
}

extern "C" int ncf_pair_rows_fill(const int64_t* rowptr, const int32_t* col, const float* val, int64_t R, const int64_t* pair_row, int64_t B,
                                  const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t capacity, const float* cand,
                                  int64_t ldcand, const float* rated, int64_t ldrated, int64_t I, int E, float atol, float rtol,
                                  int32_t* flag, ncf_stream_t stream) {
    if (R < 0 || B < 0 || capacity < 0)
        return fail(NCF_EINVAL, "ncf_pair_rows_fill: bad sizes (R %lld, B %lld, capacity %lld)", (long long)R, (long long)B, (long long)capacity);
    if (cand) {
        if (I < 0 || E < 1 || ldcand < E || ldrated < E)
            return fail(NCF_EINVAL, "ncf_pair_rows_fill: bad mask shape (I %lld, E %d, ldcand %lld, ldrated %lld)", (long long)I, E,
                        (long long)ldcand, (long long)ldrated);
        if (!(atol >= 0.f) || !(rtol >= 0.f)) return fail(NCF_EINVAL, "ncf_pair_rows_fill: atol and rtol must be >= 0");
        if (!rated && I > 0) return fail(NCF_EINVAL, "ncf_pair_rows_fill: null pointer");
    }
    if (B >= (1ll << 31)) return fail(NCF_EUNSUPPORTED, "ncf_pair_rows_fill: more than 2^31 pairs");
    if (B == 0) return NCF_OK;
    if (!rowptr || !col || !val || !pair_row || !out_rowptr || !out_col || !out_val || !flag)
        return fail(NCF_EINVAL, "ncf_pair_rows_fill: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    const bool vec = cand && E % 4 == 0 && E <= 256 && ldcand % 4 == 0 && ldrated % 4 == 0 && aligned16(cand) && aligned16(rated);
    if (!cand || I == 0)
        hipLaunchKernelGGL(pair_rows_fill_kernel<0>, grid, block, 0, s, rowptr, col, val, R, pair_row, B, out_rowptr, out_col, out_val, capacity,
                           cand, ldcand, rated, ldrated, I, E, atol, rtol, flag);
    else if (vec)
        hipLaunchKernelGGL(pair_rows_fill_kernel<1>, grid, block, 0, s, rowptr, col, val, R, pair_row, B, out_rowptr, out_col, out_val, capacity,
                           cand, ldcand, rated, ldrated, I, E, atol, rtol, flag);
    else
        hipLaunchKernelGGL(pair_rows_fill_kernel<2>, grid, block, 0, s, rowptr, col, val, R, pair_row, B, out_rowptr, out_col, out_val, capacity,
                           cand, ldcand, rated, ldrated, I, E, atol, rtol, flag);
    return check_launch("ncf_pair_rows_fill");
}
