// LightGAT training step (gnn_ncf.py:151-177): the gradient through the per-destination edge softmax over the edges a step keeps.
// (The softmax itself, ncf_gat_edge_softmax, is edge_softmax.hip's: one set of kernels for scoring and training.)  Both entries walk
// the level-0 SEGMENTS of the prepared CSR (seg_walk.h: a segment is a contiguous entry range of one row, at most seg_len long), so
// hub rows spread over many waves; split rows are finished by a per-row pass.  No float atomics, no tickets, every sum in a fixed
// order: bitwise repeatable run to run.
//
//   ncf_gat_edge_grad       g_e = attr_e <dY[row_e], drop_e(z[col_e])>,  S_r = sum_r alpha_e g_e,  dlogit_e = alpha_e (g_e - S_r).
//                           HBM-bound like the SpMM: per entry one z row (4 D bytes) + col 4 + alpha 4 + attr 4 read, g 4 written,
//                           then 12 bytes in the apply pass (g, alpha read; dlogit written).  The segment's dY row chunk stays in
//                           registers.  Lane layout of spmm_seg_kernel: LPR = D/4 lanes (rounded up to a power of two) own one row's
//                           16-byte chunks, 64/LPR entries per wave-instruction, 4 loads in flight per lane.
//                           SUMMATION ORDER (tests/gat_ref.py counts its roundings): per entry the lane's 4 products (1 mul + 3 fma),
//                           then log2(LPR) butterfly adds; S of a segment: the entry group's serial fma chain over its entries, then
//                           log2(64/LPR) butterfly adds; S of a split row: lane l adds segments l, l+64, ... in order, then a 6-step
//                           butterfly.  An entry with alpha == 0 (removed, out of range, or underflowed) reads no z row: its
//                           dlogit is 0 whatever g is.
//   ncf_gat_source_reduce   one level of ds[n] = sum over row n of the CSR by SOURCE of dlogit[eid[k]]: the segment walk of
//                           spmm_seg_kernel on scalars (a segment that is the first and last of its row writes out[row], any other
//                           its partial sum), re-applied level by level by native.gat_source_reduce as SegmentedCSR.spmm does.
#include "ncf_common.h"
#include "drop_mask.h"   // DropArgs, drop4: the message dropout mask
#include "seg_walk.h"    // wave_walk / wave_blocks, seg_row, the first / last rule, RowLanes, dispatch_lpr
#include <math.h>

namespace ncf {

// ---- gradient, pass 1: g_e into g_out[e], the segment's sum of alpha_e g_e into segsum[seg]
template <int LPR, bool DROP>
__global__ __launch_bounds__(256) void gat_edge_dot_kernel(const int64_t* __restrict__ segptr, const int32_t* __restrict__ row_of,
                                                           int64_t n_seg, int64_t n_rows, const int32_t* __restrict__ col,
                                                           const float* __restrict__ attr, const float* __restrict__ alpha,
                                                           const float* __restrict__ dY, int64_t ldy, const float* __restrict__ z,
                                                           int64_t Nz, int64_t ldz, int chunks, float* __restrict__ g_out,
                                                           float* __restrict__ segsum, DropArgs drop) {
    constexpr int EPI = RowLanes<LPR>::EPI, UNROLL = RowLanes<LPR>::UNROLL;
    const int lane = threadIdx.x & 63;
    const int c = RowLanes<LPR>::chunk(lane), eg = RowLanes<LPR>::entry(lane);
    const bool active = c < chunks;   // the chunk lies inside the row
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t s = walk.first; s < n_seg; s += walk.stride) {
        const int64_t beg = segptr[s], end = segptr[s + 1];
        const int64_t row = seg_row(row_of, s);
        f32x4 dy = {0.f, 0.f, 0.f, 0.f};
        if (active && row >= 0 && row < n_rows && end > beg) dy = *reinterpret_cast<const f32x4*>(dY + row * ldy + 4 * c);
        float sacc = 0.f;
        for (int64_t e0 = beg; e0 < end; e0 += EPI * UNROLL) {
            f32x4 v[UNROLL];
            float a[UNROLL], w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int64_t e = e0 + u * EPI + eg;
                v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                a[u] = 0.f;
                w[u] = 1.f;
                if (e < end) {
                    const float ae = alpha[e];
                    const int64_t src = col[e];
                    if (ae != 0.f && src >= 0 && src < Nz) {
                        a[u] = ae;
                        if (attr) w[u] = attr[e];
                        if (active) {
                            v[u] = *reinterpret_cast<const f32x4*>(z + src * ldz + 4 * c);
                            if (DROP) v[u] = drop4(v[u], (uint32_t)e, c, drop);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                float d = dy[0] * v[u][0];
                d = fmaf(dy[1], v[u][1], d);
                d = fmaf(dy[2], v[u][2], d);
                d = fmaf(dy[3], v[u][3], d);
#pragma unroll
                for (int off = 1; off < LPR; off <<= 1) d += __shfl_xor(d, off);
                const float g = w[u] * d;
                const int64_t e = e0 + u * EPI + eg;
                if (c == 0 && e < end) g_out[e] = g;
                sacc = fmaf(a[u], g, sacc);
            }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) sacc += __shfl_xor(sacc, off);
        if (lane == 0) segsum[s] = sacc;
    }
}

// ---- gradient, pass 2 (split rows only): S_r = the row's segment sums, lane-strided in segment order, then a butterfly
__global__ __launch_bounds__(256) void gat_row_sum_kernel(const int64_t* __restrict__ seg_first, int64_t n_rows, const float* __restrict__ segsum,
                                                          float* __restrict__ rowsum) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t r = walk.first; r < n_rows; r += walk.stride) {
        const int64_t beg = seg_first[r], end = seg_first[r + 1];
        float sm = 0.f;
        for (int64_t g = beg + lane; g < end; g += 64) sm += segsum[g];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sm += __shfl_xor(sm, off);
        if (lane == 0) rowsum[r] = sm;
    }
}

// ---- gradient, pass 3: dlogit_e = alpha_e (g_e - S_r) in place over g
__global__ __launch_bounds__(256) void gat_dlogit_kernel(const int64_t* __restrict__ segptr, const int32_t* __restrict__ row_of, int64_t n_seg,
                                                         int64_t n_rows, const float* __restrict__ alpha, const float* __restrict__ S,
                                                         float* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t sg = walk.first; sg < n_seg; sg += walk.stride) {
        const int64_t beg = segptr[sg], end = segptr[sg + 1];
        const int64_t r = seg_row(row_of, sg);                        // S is per row when rows are split, else per segment = per row
        const float Sr = (r >= 0 && r < n_rows) ? S[r] : 0.f;
        for (int64_t e = beg + lane; e < end; e += 64) {
            const float a = alpha[e];
            g[e] = a != 0.f ? a * (g[e] - Sr) : 0.f;      // an entry outside its group: +0, whatever the row's sum is
        }
    }
}

// ---- one level of the ordered reduce over the CSR by source
__global__ __launch_bounds__(256) void gat_reduce_kernel(const int64_t* __restrict__ segptr, const int32_t* __restrict__ row_of, int64_t n_seg,
                                                         const int32_t* __restrict__ idx, const float* __restrict__ val, int64_t n_val,
                                                         float* __restrict__ out, int64_t n_rows, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const WaveWalk walk = wave_walk(blockDim.x);
    for (int64_t s = walk.first; s < n_seg; s += walk.stride) {
        const int64_t beg = segptr[s], end = segptr[s + 1];
        float acc = 0.f;
        for (int64_t k = beg + lane; k < end; k += 64) {
            const int64_t id = idx ? (int64_t)idx[k] : k;
            if (id >= 0 && id < n_val) acc += val[id];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) {
            const int64_t row = seg_row(row_of, s);
            const bool first = seg_opens_row(row_of, s, row);
            const bool last = seg_closes_row(row_of, s, n_seg, row);
            if (first && last) {
                if (row >= 0 && row < n_rows) out[row] = acc;
            } else if (partial) {
                partial[s] = acc;
            }
        }
    }
}

template <int LPR>
static void launch_edge_dot(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, int64_t n_rows, const int32_t* col, const float* attr,
                            const float* alpha, const float* dY, int64_t ldy, const float* z, int64_t Nz, int64_t ldz, int chunks, float* g,
                            float* segsum, const DropArgs& d, hipStream_t s) {
    if (d.thr)
        hipLaunchKernelGGL((gat_edge_dot_kernel<LPR, true>), dim3(wave_blocks(n_seg)), dim3(256), 0, s, segptr, row_of, n_seg, n_rows, col, attr,
                           alpha, dY, ldy, z, Nz, ldz, chunks, g, segsum, d);
    else
        hipLaunchKernelGGL((gat_edge_dot_kernel<LPR, false>), dim3(wave_blocks(n_seg)), dim3(256), 0, s, segptr, row_of, n_seg, n_rows, col, attr,
                           alpha, dY, ldy, z, Nz, ldz, chunks, g, segsum, d);
}

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_gat_edge_grad_workspace_bytes(int64_t n_seg, int64_t n_rows) {
    return (size_t)((n_seg > 0 ? n_seg : 0) + (n_rows > 0 ? n_rows : 0)) * sizeof(float);
}

extern "C" int ncf_gat_edge_grad(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, const int64_t* seg_first, int64_t n_rows,
                                 const int32_t* col, const float* attr, const float* alpha, const float* dY, int64_t ldy, const float* z,
                                 int64_t Nz, int64_t ldz, int D, float p, uint32_t seed, float* dlogit_out, void* workspace,
                                 size_t workspace_bytes, ncf_stream_t stream) {
    if (n_rows < 0 || n_seg < 0 || Nz < 0 || D <= 0) return fail(NCF_EINVAL, "ncf_gat_edge_grad: bad size");
    if (D % 4) return fail(NCF_EINVAL, "ncf_gat_edge_grad: D = %d (need D %% 4 == 0)", D);
    if (D > 256) return fail(NCF_EUNSUPPORTED, "ncf_gat_edge_grad: D = %d (need D <= 256)", D);
    if (!isfinite(p) || !(p >= 0.f && p < 1.f)) return fail(NCF_EINVAL, "ncf_gat_edge_grad: p = %g is not in [0, 1)", (double)p);
    if (!row_of && n_seg != n_rows) return fail(NCF_EINVAL, "ncf_gat_edge_grad: without row_of the segments are the rows");
    if (n_rows == 0 || n_seg == 0) return NCF_OK;
    if (!segptr || !col || !alpha || !dY || !z || !dlogit_out || !workspace || (row_of && !seg_first))
        return fail(NCF_EINVAL, "ncf_gat_edge_grad: null pointer");
    if (ldy % 4 || ldz % 4 || ldy < D || ldz < D || !aligned16(dY) || !aligned16(z))
        return fail(NCF_EINVAL, "ncf_gat_edge_grad: rows must be 16-byte aligned (ld %% 4 == 0, ld >= D)");
    if (workspace_bytes < ncf_gat_edge_grad_workspace_bytes(n_seg, n_rows)) return fail(NCF_EWORKSPACE, "ncf_gat_edge_grad: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* segsum = (float*)workspace;
    float* rowsum = segsum + n_seg;
    const DropArgs d = drop_args(nullptr, seed, p);
    const int chunks = D / 4;
    dispatch_lpr(chunks, [&](auto lpr) {
        launch_edge_dot<decltype(lpr)::value>(segptr, row_of, n_seg, n_rows, col, attr, alpha, dY, ldy, z, Nz, ldz, chunks, dlogit_out, segsum, d, st);
    });
    if (row_of) hipLaunchKernelGGL(gat_row_sum_kernel, dim3(wave_blocks(n_rows)), dim3(256), 0, st, seg_first, n_rows, segsum, rowsum);
    hipLaunchKernelGGL(gat_dlogit_kernel, dim3(wave_blocks(n_seg)), dim3(256), 0, st, segptr, row_of, n_seg, n_rows, alpha, row_of ? rowsum : segsum,
                       dlogit_out);
    return check_launch("ncf_gat_edge_grad");
}

extern "C" int ncf_gat_source_reduce(const int64_t* segptr, const int32_t* row_of, int64_t n_seg, const int32_t* idx, const float* val,
                                     int64_t n_val, float* out, int64_t n_rows, float* partial, ncf_stream_t stream) {
    if (n_seg < 0 || n_val < 0 || n_rows < 0) return fail(NCF_EINVAL, "ncf_gat_source_reduce: negative size");
    if (!row_of && n_seg != n_rows) return fail(NCF_EINVAL, "ncf_gat_source_reduce: without row_of the segments are the rows");
    if (n_seg == 0) return NCF_OK;
    if (!segptr || !out || (n_val > 0 && !val)) return fail(NCF_EINVAL, "ncf_gat_source_reduce: null pointer");
    hipLaunchKernelGGL(gat_reduce_kernel, dim3(wave_blocks(n_seg)), dim3(256), 0, (hipStream_t)stream, segptr, row_of, n_seg, idx, val, n_val, out,
                       n_rows, partial);
    return check_launch("ncf_gat_source_reduce");
}
