// Item-item attention statistics of an evaluation file from the logit table: for every sample (user u, candidate c) and every
// valid entry e of u's rated set, sum[c, col_e] += the attention weight of col_e towards c (float64) and count[c, col_e] += 1 —
// the two (n_items, n_items) tables the reference's eval_model builds on the host from a dense (batch, catalogue) weight matrix
// (eval.py:101-108, 137-143).  ncf_attn_logits' table ST (attn_cross.hip) holds every logit: a sample's weights are a column
// lookup over its user's row and a softmax (attn_table.h).
//
// Two launches inside the one entry:
//   attn_stats_softmax_kernel  one wave = one sample, four samples per workgroup, no barrier.  The column softmax of attn_table.h,
//       which attn_explain_kernel calls too (m_s and l_s have attn_explain's bits), written as (m_s, l_s) to the workspace, 8 bytes
//       per sample.  Sets the sticky flag for a user row or candidate out of range.
//   attn_stats_accumulate_kernel  owner computes: one wave (= one workgroup) owns (candidate c, slab of kStSlab columns of the
//       rated axis) and nobody else touches those cells.  Its accumulators — kStSlab doubles and kStSlab int64 — live in LDS,
//       are initialised from the caller's tables and written back at the end.  The wave walks c's samples in the order the caller's
//       (order, cand_rowptr) lists them (ascending sample index), 64 samples' headers fetched at a time (lane j holds sample j's
//       row bounds, m and l; they are broadcast with readlane), and for each sample its lanes stride over the row's entries, skip the
//       columns outside the slab and add w = exp_le0(ST[col, c] - m) / l into the slab's cells.  The chain of one candidate is
//       serial, so what a sample costs is memory round trips: the columns of kStBatch stripes (512 entries) are loaded together,
//       then their table lookups together, and the next sample's first columns are requested before this sample's lookups are
//       waited for.  Valid columns of one row are distinct (the documented precondition), so within a sample no two lanes touch
//       one cell; between samples the wave's LDS accesses are ordered by wave_lds_sync (fence + wave barrier).  A repeated column
//       cannot fault: the lanes race for one LDS cell of their own wave and one of them wins.
// No atomics: the additions into a cell happen in the listed order starting from the value already in the table, so two calls
// give the same bits and a file accumulated in two calls (first half, then second half) gives the bits of one call.  Every loop
// is bounded by S or by a row's length.
#include "attn_table.h"
#include "topk_common.h"

namespace ncf {

constexpr int kStWaves = 4;            // samples per workgroup of the softmax kernel
constexpr int kStSlab = 512;           // rated columns owned by one wave of the accumulation kernel
constexpr int kStBatch = 8;            // stripes of 64 entries whose loads the accumulation kernel keeps in flight together

__global__ __launch_bounds__(kStWaves* kWave) void attn_stats_softmax_kernel(
    const float* __restrict__ st, int64_t ldst, int64_t Ir, int64_t Ic, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, int64_t n_rows, const int64_t* __restrict__ user_rows, const int64_t* __restrict__ cands,
    int64_t S, float2* __restrict__ ml, int32_t* __restrict__ oob) {
    __shared__ float caches[kStWaves][kTableCache];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t s = (int64_t)blockIdx.x * kStWaves + wave;
    if (s >= S) return;                                                // wave-uniform; the kernel has no barrier
    const int64_t row = user_rows[s], c = cands[s];
    const bool live = row >= 0 && row < n_rows && c >= 0 && c < Ic;
    if (oob && lane == 0 && !live) *oob = 1;                           // sticky
    const int64_t beg = live ? rowptr[row] : 0, end = live ? rowptr[row + 1] : 0;
    const TableColumn tc{st + (live ? c : 0), ldst, Ir, col, beg, end, caches[wave], lane};
    const float m = tc.max();
    const float l = tc.denominator(m);
    if (lane == 0) ml[s] = make_float2(m, l);
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int j) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, j), hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kWave) void attn_stats_accumulate_kernel(
    const float* __restrict__ st, int64_t ldst, int64_t Ir, int64_t Ic, int64_t n_slabs, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, int64_t n_rows, const int64_t* __restrict__ user_rows, const int64_t* __restrict__ cands,
    int64_t S, const int64_t* __restrict__ order, const int64_t* __restrict__ cand_rowptr, const float2* __restrict__ ml,
    double* __restrict__ sum, int64_t ldsum, int64_t* __restrict__ count, int64_t ldcount) {
    __shared__ double acc[kStSlab];
    __shared__ long long cnt[kStSlab];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x / n_slabs, slab = (int64_t)blockIdx.x % n_slabs;
    if (c >= Ic) return;
    // the candidate's samples are order[k0 .. k1); whatever the two arrays hold, nothing outside [0, S) is read
    int64_t k0 = cand_rowptr[c], k1 = cand_rowptr[c + 1];
    k0 = k0 < 0 ? 0 : (k0 > S ? S : k0);
    k1 = k1 < k0 ? k0 : (k1 > S ? S : k1);
    if (k0 == k1) return;                                              // no sample: the cells keep the caller's values
    const int64_t lo = slab * kStSlab;
    const int width = (int)(Ir - lo < kStSlab ? Ir - lo : kStSlab);
    double* __restrict__ srow = sum + c * ldsum + lo;
    int64_t* __restrict__ crow = count + c * ldcount + lo;
    for (int i = lane; i < width; i += kWave) {
        acc[i] = srow[i];
        cnt[i] = crow[i];
    }
    wave_lds_sync();
    const float* __restrict__ stc = st + c;

    // the columns of entries e0 + 64 u + lane, u < kStBatch, of a row that ends at t (-1 past the end): kStBatch loads in flight
    auto load_cols = [&](int64_t e0, int64_t t, int(&cc)[kStBatch]) {
#pragma unroll
        for (int u = 0; u < kStBatch; ++u) {
            const int64_t e = e0 + u * kWave + lane;
            cc[u] = e < t ? col[e] : -1;
        }
    };
    // the weights of those entries towards c, added into the cells of this slab; the kStBatch table lookups are in flight together
    auto add = [&](const int(&cc)[kStBatch], bool any, float mj, float lj) {
        float v[kStBatch];
#pragma unroll
        for (int u = 0; u < kStBatch; ++u) {
            const int64_t i = (int64_t)cc[u] - lo;                     // 0 <= i < width: a valid column (lo + width <= I_r) of this slab
            v[u] = (any && i >= 0 && i < width) ? stc[(int64_t)cc[u] * ldst] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < kStBatch; ++u) {
            const int64_t i = (int64_t)cc[u] - lo;
            if (i >= 0 && i < width) {
                float w = 0.f;
                if (any) {
                    w = exp_le0(v[u] - mj) / lj;
                    w = w == w ? w : 0.f;                              // the reference's NaN -> 0
                }
                acc[i] += (double)w;
                cnt[i] += 1;                                           // structural: a valid stored entry always counts
            }
        }
    };

    for (int64_t kb = k0; kb < k1; kb += kWave) {
        // lane j: the header of sample order[kb + j]; a sample that is not this candidate's, or whose row is out of range, is empty
        int64_t beg = 0, end = 0;
        float m = -INFINITY, l = 0.f;
        if (kb + lane < k1) {
            const int64_t s = order[kb + lane];
            if (s >= 0 && s < S && cands[s] == c) {
                const int64_t row = user_rows[s];
                if (row >= 0 && row < n_rows) {
                    beg = rowptr[row];
                    end = rowptr[row + 1];
                    const float2 v = ml[s];
                    m = v.x;
                    l = v.y;
                }
            }
        }
        const int n = (int)(k1 - kb < kWave ? k1 - kb : kWave);
        int pre[kStBatch];                                             // the first columns of the sample about to be added
        load_cols(readlane64(beg, 0), readlane64(end, 0), pre);
        for (int j = 0; j < n; ++j) {                                  // ascending position in the list: ascending sample index
            const int64_t b = readlane64(beg, j), t = readlane64(end, j);
            const float mj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), j));
            const float lj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), j));
            const bool any = mj != -INFINITY && lj > 0.f;              // false: no finite logit, or a zero / NaN denominator -> w = 0
            int nxt[kStBatch];                                         // the next sample's first columns travel behind this one's logits
            const int jn = j + 1 < n ? j + 1 : j;
            load_cols(readlane64(beg, jn), readlane64(end, jn), nxt);
            add(pre, any, mj, lj);
            for (int64_t e0 = b + kStBatch * kWave; e0 < t; e0 += kStBatch * kWave) {
                int cc[kStBatch];
                load_cols(e0, t, cc);
                add(cc, any, mj, lj);
            }
            wave_lds_sync();                                           // the next sample's lanes may own other cells of the same slab
#pragma unroll
            for (int u = 0; u < kStBatch; ++u) pre[u] = nxt[u];
        }
    }
    for (int i = lane; i < width; i += kWave) {
        srow[i] = acc[i];
        crow[i] = cnt[i];
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_attn_stats_workspace_bytes(int64_t S) { return S > 0 ? (size_t)S * sizeof(float2) : 0; }

extern "C" int ncf_attn_stats(const float* st, int64_t ldst, int64_t Ir, int64_t Ic, const int64_t* rowptr, const int32_t* col,
                              int64_t n_rows, const int64_t* user_rows, const int64_t* cands, int64_t S, const int64_t* order,
                              const int64_t* cand_rowptr, double* sum, int64_t ldsum, int64_t* count, int64_t ldcount, int32_t* oob,
                              void* workspace, size_t workspace_bytes, ncf_stream_t stream) {
    if (Ir < 0 || Ic < 0 || n_rows < 0 || S < 0) return fail(NCF_EINVAL, "ncf_attn_stats: bad sizes");
    if (S == 0) return NCF_OK;
    const int64_t n_slabs = (Ir + kStSlab - 1) / kStSlab;
    if (Ir > 0x7FFFFFFF || (n_slabs > 0 && Ic > (int64_t)0x7FFFFFFF / n_slabs))
        return fail(NCF_EUNSUPPORTED, "ncf_attn_stats: I_r = %lld, I_c = %lld is out of range (int32 columns, 2^31 - 1 workgroups)",
                    (long long)Ir, (long long)Ic);
    if (S > (int64_t)0x7FFFFFFF * kStWaves) return fail(NCF_EUNSUPPORTED, "ncf_attn_stats: more than 2^31 - 1 workgroups");
    if ((!st && Ir > 0 && Ic > 0) || !rowptr || !user_rows || !cands || !order || !cand_rowptr)
        return fail(NCF_EINVAL, "ncf_attn_stats: null pointer");
    if ((!sum || !count) && Ir > 0 && Ic > 0) return fail(NCF_EINVAL, "ncf_attn_stats: null output pointer");
    if (!workspace) return fail(NCF_EINVAL, "ncf_attn_stats: null workspace");
    if (!aligned(st, 4) || !aligned(col, 4) || !aligned(oob, 4) || !aligned(rowptr, 8) || !aligned(user_rows, 8) || !aligned(cands, 8) ||
        !aligned(order, 8) || !aligned(cand_rowptr, 8) || !aligned(sum, 8) || !aligned(count, 8) || !aligned(workspace, 8))
        return fail(NCF_EINVAL, "ncf_attn_stats: misaligned pointer");
    if (ldst < Ic) return fail(NCF_EINVAL, "ncf_attn_stats: leading dimension of the logit table smaller than its row");
    if (ldsum < Ir || ldcount < Ir) return fail(NCF_EINVAL, "ncf_attn_stats: leading dimension of sum / count smaller than I_r");
    if (workspace_bytes < ncf_attn_stats_workspace_bytes(S))
        return fail(NCF_EWORKSPACE, "ncf_attn_stats: workspace of %zu bytes, %zu needed", workspace_bytes, ncf_attn_stats_workspace_bytes(S));
    float2* ml = (float2*)workspace;
    const int64_t grid = (S + kStWaves - 1) / kStWaves;
    hipLaunchKernelGGL(attn_stats_softmax_kernel, dim3((unsigned)grid), dim3(kStWaves * kWave), 0, (hipStream_t)stream, st, ldst, Ir, Ic,
                       rowptr, col, n_rows, user_rows, cands, S, ml, oob);
    int rc = check_launch("ncf_attn_stats");
    if (rc != NCF_OK || Ic == 0 || Ir == 0) return rc;
    hipLaunchKernelGGL(attn_stats_accumulate_kernel, dim3((unsigned)(Ic * n_slabs)), dim3(kWave), 0, (hipStream_t)stream, st, ldst, Ir, Ic,
                       n_slabs, rowptr, col, n_rows, user_rows, cands, S, order, cand_rowptr, ml, sum, ldsum, count, ldcount);
    return check_launch("ncf_attn_stats");
}
