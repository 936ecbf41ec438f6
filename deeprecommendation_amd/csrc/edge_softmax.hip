// LightGAT edge attention (gnn_ncf.py:151-177 with PyG softmax), the ONE edge softmax of the library: for destination row r,
//   alpha_e = exp(s[col_e] - max_r) / (sum_r exp(s[col_.] - max_r) + 1e-16),   coef_e = (attr ? attr_e : 1) * alpha_e
// over the entries of r that COUNT: col_e in range AND (keep == NULL or keep_e != 0).  An entry that does not count gets 0.
// s[n] = w_j . x[n] is the SOURCE half of AttNet(cat(x_j, x_i)); the destination half w_i . x_i + b is constant inside a softmax
// group and cancels.  4-byte scalars only (col, keep, s gathered from an N-float table, L2-resident).
//
// Two forms, both without atomics and in a fixed order (bitwise repeatable):
//   row form        one wave per row, three walks: max, sum of expf(s - max), apply.
//   segmented form  over the level-0 SEGMENTS of the prepared CSR (rows longer than seg_len entries are split; a hub item of BASELINE
//                   config 4 has 4 M in-edges: one wave walking them three times is ~0.2 s, the whole 100 M-edge graph otherwise
//                   ~1 ms).  Three passes, every one parallel over segments or rows:
//                     1. per segment (one wave):  m_seg = max s[col_e],  l_seg = sum exp(s[col_e] - m_seg)
//                     2. per row (one wave over its segments [seg_first[r], seg_first[r+1])):  M = max m_seg,  L = sum l_seg exp(m_seg - M)
//                     3. per segment:  alpha_e = exp(s[col_e] - M_row) / (L_row + 1e-16)
// Operation order: the lane's strided max, a butterfly from offset 32 down to 1, expf(s - max) summed per lane, the same butterfly,
// + 1e-16f, attr[e] * a.  Three ABI entries call it, each with its own argument checks: ncf_edge_softmax_csr (row form),
// ncf_edge_softmax_segmented, and ncf_gat_edge_softmax (either form, with keep and alpha).
#include "ncf_common.h"
#include "seg_walk.h"
#include <math.h>

namespace ncf {

// TRAIN picks one of two instantiations at compile time.  false scores (ncf_edge_softmax_csr / _segmented): no keep indicator, out
// only — the kernels the scoring path always had.  true trains (ncf_gat_edge_softmax): a keep indicator (NULL: every entry kept),
// alpha written, out only when there are weights, and the segment's row range-checked in the apply pass.  As run-time pointers in one
// instantiation these choices cost the scoring softmax 2 to 6 %, the range check alone 0.3 %.
template <bool TRAIN>
__device__ __forceinline__ bool softmax_counts(const int32_t* __restrict__ col, const float* __restrict__ keep, int64_t e, int64_t Ns,
                                               int64_t& c) {
    c = col[e];
    return c >= 0 && c < Ns && (!TRAIN || !keep || keep[e] != 0.f);
}

// max and sum of exp(s - max) over the counting entries of [beg, end), in every lane
template <bool TRAIN>
__device__ __forceinline__ void softmax_stats(const int32_t* __restrict__ col, const float* __restrict__ keep, const float* __restrict__ s,
                                              int64_t Ns, int64_t beg, int64_t end, int lane, float& mx, float& sm) {
    mx = -INFINITY;
    for (int64_t e = beg + lane; e < end; e += 64) {
        int64_t c;
        if (softmax_counts<TRAIN>(col, keep, e, Ns, c)) mx = fmaxf(mx, s[c]);
    }
    mx = wave_max(mx);
    sm = 0.f;
    for (int64_t e = beg + lane; e < end; e += 64) {
        int64_t c;
        if (softmax_counts<TRAIN>(col, keep, e, Ns, c)) sm += expf(s[c] - mx);
    }
    sm = wave_sum(sm);
}

// alpha and out = (attr ? attr : 1) * alpha of [beg, end) under the row's max and denominator
template <bool TRAIN>
__device__ __forceinline__ void softmax_apply(const int32_t* __restrict__ col, const float* __restrict__ attr, const float* __restrict__ keep,
                                              const float* __restrict__ s, int64_t Ns, int64_t beg, int64_t end, int lane, bool row_ok,
                                              float mx, float den, float* __restrict__ alpha, float* __restrict__ out) {
    for (int64_t e = beg + lane; e < end; e += 64) {
        int64_t c;
        const float a = (softmax_counts<TRAIN>(col, keep, e, Ns, c) && row_ok) ? expf(s[c] - mx) / den : 0.f;
        if (TRAIN) {
            alpha[e] = a;
            if (out) out[e] = attr[e] * a;         // out is NULL without weights: coef is alpha
        } else {
            out[e] = attr ? attr[e] * a : a;       // weight * a_scores * W(x_j), :174 / :176
        }
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void edge_softmax_row_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                               const float* __restrict__ attr, const float* __restrict__ keep,
                                                               const float* __restrict__ s, int64_t n_rows, int64_t Ns,
                                                               float* __restrict__ alpha, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t r = walk.first; r < n_rows; r += walk.stride) {
        const int64_t beg = rowptr[r], end = rowptr[r + 1];
        float mx, sm;
        softmax_stats<TRAIN>(col, keep, s, Ns, beg, end, lane, mx, sm);
        softmax_apply<TRAIN>(col, attr, keep, s, Ns, beg, end, lane, true, mx, sm + 1e-16f, alpha, out);
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void edge_softmax_seg_stats_kernel(const int64_t* __restrict__ segptr, int64_t n_seg, const int32_t* __restrict__ col,
                                                                     const float* __restrict__ keep, const float* __restrict__ s, int64_t Ns,
                                                                     float* __restrict__ segm, float* __restrict__ segl) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t g = walk.first; g < n_seg; g += walk.stride) {
        float mx, sm;
        softmax_stats<TRAIN>(col, keep, s, Ns, segptr[g], segptr[g + 1], lane, mx, sm);
        if (lane == 0) { segm[g] = mx; segl[g] = sm; }
    }
}

__global__ __launch_bounds__(256) void edge_softmax_row_stats_kernel(const int64_t* __restrict__ seg_first, int64_t n_rows, const float* __restrict__ segm,
                                                                     const float* __restrict__ segl, float* __restrict__ rowm, float* __restrict__ rowden) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t r = walk.first; r < n_rows; r += walk.stride) {
        const int64_t beg = seg_first[r], end = seg_first[r + 1];
        float mx = -INFINITY;
        for (int64_t g = beg + lane; g < end; g += 64) mx = fmaxf(mx, segm[g]);
        mx = wave_max(mx);
        float sm = 0.f;
        for (int64_t g = beg + lane; g < end; g += 64) {
            const float m = segm[g];
            if (m != -INFINITY) sm += segl[g] * expf(m - mx);
        }
        sm = wave_sum(sm);
        if (lane == 0) { rowm[r] = mx; rowden[r] = sm + 1e-16f; }
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void edge_softmax_seg_apply_kernel(const int64_t* __restrict__ segptr, const int32_t* __restrict__ row_of, int64_t n_seg,
                                                                     int64_t n_rows, const int32_t* __restrict__ col, const float* __restrict__ attr,
                                                                     const float* __restrict__ keep, const float* __restrict__ s, int64_t Ns,
                                                                     const float* __restrict__ rowm, const float* __restrict__ rowden,
                                                                     float* __restrict__ alpha, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t g = walk.first; g < n_seg; g += walk.stride) {
        const int64_t r = row_of[g];
        const bool row_ok = !TRAIN || (r >= 0 && r < n_rows);
        const float mx = row_ok ? rowm[r] : 0.f, den = row_ok ? rowden[r] : 1.f;
        softmax_apply<TRAIN>(col, attr, keep, s, Ns, segptr[g], segptr[g + 1], lane, row_ok, mx, den, alpha, out);
    }
}

static size_t softmax_workspace_bytes(int64_t n_seg, int64_t n_rows) {   // m and l per segment, M and L + 1e-16 per row
    return (size_t)(2 * (n_seg > 0 ? n_seg : 0) + 2 * (n_rows > 0 ? n_rows : 0)) * sizeof(float);
}

template <bool TRAIN>
static void softmax_rows(const int64_t* rowptr, const int32_t* col, const float* attr, const float* keep, const float* s, int64_t n_rows,
                         int64_t Ns, float* alpha, float* out, hipStream_t st) {
    hipLaunchKernelGGL(edge_softmax_row_kernel<TRAIN>, dim3(wave_blocks(n_rows)), dim3(256), 0, st, rowptr, col, attr, keep, s, n_rows, Ns, alpha, out);
}

template <bool TRAIN>
static void softmax_segments(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, const int64_t* seg_first, int64_t n_rows,
                             const int32_t* col, const float* attr, const float* keep, const float* s, int64_t Ns, float* alpha, float* out,
                             void* workspace, hipStream_t st) {
    float* segm = (float*)workspace;
    float* segl = segm + n_seg;
    float* rowm = segl + n_seg;
    float* rowden = rowm + n_rows;
    hipLaunchKernelGGL(edge_softmax_seg_stats_kernel<TRAIN>, dim3(wave_blocks(n_seg)), dim3(256), 0, st, segptr, n_seg, col, keep, s, Ns, segm, segl);
    hipLaunchKernelGGL(edge_softmax_row_stats_kernel, dim3(wave_blocks(n_rows)), dim3(256), 0, st, seg_first, n_rows, segm, segl, rowm, rowden);
    hipLaunchKernelGGL(edge_softmax_seg_apply_kernel<TRAIN>, dim3(wave_blocks(n_seg)), dim3(256), 0, st, segptr, row_of, n_seg, n_rows, col, attr, keep, s,
                       Ns, rowm, rowden, alpha, out);
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_edge_softmax_csr(const int64_t* rowptr, const int32_t* col, const float* attr, const float* s, int64_t n_rows,
                                    int64_t Ns, float* out, ncf_stream_t stream) {
    if (n_rows < 0 || Ns < 0) return fail(NCF_EINVAL, "ncf_edge_softmax_csr: bad sizes");
    if (n_rows == 0) return NCF_OK;
    if (!rowptr || !s) return fail(NCF_EINVAL, "ncf_edge_softmax_csr: null pointer");
    softmax_rows<false>(rowptr, col, attr, nullptr, s, n_rows, Ns, nullptr, out, (hipStream_t)stream);
    return check_launch("ncf_edge_softmax_csr");
}

extern "C" size_t ncf_edge_softmax_segmented_workspace_bytes(int64_t n_seg, int64_t n_rows) { return softmax_workspace_bytes(n_seg, n_rows); }

extern "C" int ncf_edge_softmax_segmented(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, const int64_t* seg_first, int64_t n_rows,
                                          const int32_t* col, const float* attr, const float* s, int64_t Ns, float* out, void* workspace,
                                          size_t workspace_bytes, ncf_stream_t stream) {
    if (n_rows < 0 || n_seg < 0 || Ns < 0) return fail(NCF_EINVAL, "ncf_edge_softmax_segmented: bad sizes");
    if (n_rows == 0 || n_seg == 0) return NCF_OK;
    if (!segptr || !row_of || !seg_first || !s || !workspace) return fail(NCF_EINVAL, "ncf_edge_softmax_segmented: null pointer");
    if (workspace_bytes < softmax_workspace_bytes(n_seg, n_rows)) return fail(NCF_EWORKSPACE, "ncf_edge_softmax_segmented: workspace too small");
    softmax_segments<false>(segptr, row_of, n_seg, seg_first, n_rows, col, attr, nullptr, s, Ns, nullptr, out, workspace, (hipStream_t)stream);
    return check_launch("ncf_edge_softmax_segmented");
}

extern "C" size_t ncf_gat_edge_softmax_workspace_bytes(int64_t n_seg, int64_t n_rows) { return softmax_workspace_bytes(n_seg, n_rows); }

extern "C" int ncf_gat_edge_softmax(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, const int64_t* seg_first, int64_t n_rows,
                                    const int32_t* col, const float* attr, const float* keep, const float* s, int64_t Ns, float* alpha_out,
                                    float* coef_out, void* workspace, size_t workspace_bytes, ncf_stream_t stream) {
    if (n_rows < 0 || n_seg < 0 || Ns < 0) return fail(NCF_EINVAL, "ncf_gat_edge_softmax: negative size");
    if (!row_of && n_seg != n_rows) return fail(NCF_EINVAL, "ncf_gat_edge_softmax: without row_of the segments are the rows");
    if (n_rows == 0 || n_seg == 0) return NCF_OK;
    if (!segptr || !col || !s || !alpha_out || (attr && !coef_out) || (row_of && (!seg_first || !workspace)))
        return fail(NCF_EINVAL, "ncf_gat_edge_softmax: null pointer");
    if (row_of && workspace_bytes < softmax_workspace_bytes(n_seg, n_rows))
        return fail(NCF_EWORKSPACE, "ncf_gat_edge_softmax: workspace too small");
    float* coef = attr ? coef_out : nullptr;   // without weights coef is alpha: one store per entry
    if (!row_of) softmax_rows<true>(segptr, col, attr, keep, s, n_rows, Ns, alpha_out, coef, (hipStream_t)stream);
    else softmax_segments<true>(segptr, row_of, n_seg, seg_first, n_rows, col, attr, keep, s, Ns, alpha_out, coef, workspace, (hipStream_t)stream);
    return check_launch("ncf_gat_edge_softmax");
}
