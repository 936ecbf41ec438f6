// NeuMF (He et al. 2017): the MLP tower and the GMF branch under one output layer, scored in one wave.
//     score = predict(cat(p (.) q, phi)) = fl(fl(s_mlp + g) + bl)
// s_mlp: the fused MLP scorer's 1-wide last layer over the tower's last hidden activation phi, without its bias, with
// predict.weight[:, D:] as that layer's weights.  Layer 1 starts from b1 and takes its k-steps q ascending (the user table's, then the
// item table's), tiles nt-major, j ascending; layer 2 and the last sum are mlp_fused.h's fused_layer2 and fused_last_sum, not copies:
// the bits are those of ncf_score_fused for the pair with the same blob and a zero last bias.
// g: the GMF term over the second pair of tables with w = predict.weight[0, :D] (gmf.h has its operation order and why it is never
// -0.0).  s_mlp is never -0.0 either (mlp_topk.h), so fl(s_mlp + g) is not, and the score is -0.0 only if that sum and bl both are:
// the key round trip of the ranking entries (topk_map / topk_unmap) returns the caller's bits for every non-NaN score.
//   ncf_neumf_score              pairs: one wave per 32-pair tile, four independent waves per workgroup, one launch form.  The first
//                                chunks of the pair's GMF rows are requested before layer 2 and land under its MFMAs; the term costs
//                                3 D / 2 VALU operations per lane against the tile's 768 - 1024 MFMAs.
//   ncf_neumf_topk / _rank       users first: mlp_topk.h's waves and entry bodies with the GMF term on (GmfArgs).  The prefix pass is
//                                followed by gmf_trow_kernel, which writes every listed user's rounded w (.) p row behind the prefix
//                                state; a wave holds its user's row in LDS and adds g to s_mlp before the sink.
#include "mlp_topk.h"

namespace ncf {

struct NeumfArgs {
    const float* tabA; int64_t rowsU; int64_t ldA;   // the tower's user table (EA wide) and the users' GMF table (D wide): rowsU rows
    const float* tabB; int64_t rowsI; int64_t ldB;   // the items' two tables
    const float* tabP; int64_t ldP;
    const float* tabQ; int64_t ldQ;
    const int64_t* idxU; const int64_t* idxI;
    int64_t B; int EA; int D;
    const float* Wp1; const float* b1; const float* Wp2; const float* b2; const float* wl; const float* bl;
    const float* w;
    float* out; int32_t* oob;
};

template <int K0, int N1, int N2>
__global__ __launch_bounds__(256, 2) void neumf_score_kernel(NeumfArgs a) {
    constexpr int NT1 = N1 / 32, Q1 = K0 / 8;
    constexpr int AHEAD = N1 >= 256 ? 4 : 8;         // GMF chunks in flight under layer 2 (8 VGPRs each): what the registers leave
    const int lane = threadIdx.x & 63;
    const int m = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 32 >= a.B) return;                    // whole wave exits together
    const int64_t p = tile * 32 + m;
    const int64_t pc = p < a.B ? p : a.B - 1;
    // an id outside its table reads row 0 of both of that side's tables as zeros
    const int64_t iu = a.idxU ? a.idxU[pc] : pc, ii = a.idxI ? a.idxI[pc] : pc;
    const bool okU = (iu >= 0) & (iu < a.rowsU), okI = (ii >= 0) & (ii < a.rowsI);
    if (!(okU & okI) && a.oob) *a.oob = 1;
    const int64_t ru = okU ? iu : 0, ri = okI ? ii : 0;
    const float* rowA = a.tabA + ru * a.ldA + 4 * h;
    const float* rowB = a.tabB + ri * a.ldB + 4 * h;
    const float* prow = a.tabP + ru * a.ldP + 4 * h;
    const float* qrow = a.tabQ + ri * a.ldQ + 4 * h;
    const float zA = fused_zmul(okU), zB = fused_zmul(okI);
    const int qa = a.EA / 8, nS = a.D / 8;

    // ---- layer 1: acc1 = b1 + W1 . X^T, every k-step in order (mlp_prefix_kernel's loop over the whole concat) ----
    f32x16 acc1[NT1];
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) fused_load_tile(acc1[nt], a.b1, nt, h);
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.Wp1) + lane;
#pragma unroll
    for (int q = 0; q < Q1; ++q) {
        const f32x4 xb = fused_ldg4(q < qa ? rowA + 8 * q : rowB + 8 * (q - qa)) * (q < qa ? zA : zB);
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) {
            const f32x4 w = wp[(q * NT1 + nt) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], xb[j], acc1[nt], 0, 0, 0);
        }
    }

    // ---- the GMF rows' first chunks: requested here, used after the last layer ----
    f32x4 ppre[AHEAD], qpre[AHEAD];
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) {
        ppre[s] = fused_ldg4(prow + 8 * min(s, nS - 1));
        qpre[s] = fused_ldg4(qrow + 8 * min(s, nS - 1));
    }

    float s_mlp;
    if constexpr (N2 > 0) {
        f32x16 acc2[N2 / 32];
        fused_layer2<N1, N2>(acc1, acc2, a.b2, a.Wp2, lane);
        s_mlp = fused_last_sum(acc2, a.wl, lane);
    } else {
        s_mlp = fused_last_sum(acc1, a.wl, lane);
    }
    const float g = gmf_dot_pair(a.w + 4 * h, prow, okU, qrow, okI, nS, ppre, qpre);
    const float score = (s_mlp + g) + a.bl[0];
    if (h == 0 && p < a.B) a.out[p] = score;
}

// The t rows of n listed users for the full-catalogue entries: trow[r][d] = fl(w[d] * p[d]) with p the GMF row of user idx[r] (r with
// idx NULL), zeros for an id outside the table (which sets the flag).  One thread per chunk of four.
__global__ __launch_bounds__(256) void gmf_trow_kernel(const float* __restrict__ tabP, int64_t rows, int64_t ld,
                                                       const int64_t* __restrict__ idx, int64_t n, int D, const float* __restrict__ w,
                                                       float* __restrict__ trow, int32_t* oob) {
    const int cpr = D / 4;                            // chunks per row
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * cpr) return;
    const int64_t r = i / cpr;
    const int c = (int)(i % cpr);
    const int64_t iu = idx ? idx[r] : r;
    const bool ok = (iu >= 0) & (iu < rows);
    if (!ok && oob) *oob = 1;
    const f32x4 p = gmf_row(fused_ldg4(tabP + (ok ? iu : 0) * ld + 4 * c), ok);
    *reinterpret_cast<f32x4*>(trow + r * D + 4 * c) = gmf_t(fused_ldg4(w + 4 * c), p);
}

// The GMF term of the two full-catalogue entries, as mlp_topk.h's bodies take it (MlpNoGmf there is the empty one).
struct NeumfGmf {
    typedef GmfArgs<MtArgs> TopkArgs;
    typedef GmfArgs<MrArgs> RankArgs;
    const float* tabP; int64_t ldP; const float* tabQ; int64_t ldQ; int D; const float* w;

    size_t extra_bytes(int64_t rows) const { return (size_t)rows * D * sizeof(float); }   // D % 8 == 0: a multiple of 32 bytes
    int check(const char* what, int64_t rows, int user_first) const {
        if (!gmf_width_ok(D)) return fail(NCF_EUNSUPPORTED, "%s: D = %d is not a multiple of 8 in 8 .. %d", what, D, kGmfMaxD);
        if (!user_first) return fail(NCF_EUNSUPPORTED, "%s: users first only", what);
        if (rows == 0) return NCF_OK;
        if (!tabP || !tabQ || !w) return fail(NCF_EINVAL, "%s: null argument", what);
        if (ldP < D || ldQ < D || ldP % 4 || ldQ % 4 || !aligned16(tabP) || !aligned16(tabQ) || !aligned16(w))
            return fail(NCF_EINVAL, "%s: GMF tables and w must be 16-byte aligned with ld %% 4 == 0 and ld >= D", what);
        return NCF_OK;
    }
    template <class A>
    void prepare(A& a, void* extra, int64_t rowsU, const int64_t* user_ids, int64_t rows, int32_t* oob, hipStream_t s) const {
        const int64_t chunks = rows * (D / 4);
        hipLaunchKernelGGL(gmf_trow_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, tabP, rowsU, ldP, user_ids, rows, D, w,
                           (float*)extra, oob);
        a.tabQ = tabQ; a.ldQ = ldQ;
        a.trow = (const float*)extra; a.D = D;
    }
};

static bool neumf_shape_ok(int dtype, int EA, int EB, int D, int n_layers, const int* dims) {
    return mt_shape_ok(dtype, EA, EB, n_layers, dims) && gmf_width_ok(D);
}

static int neumf_score_launch(const char* what, int dtype, const void* tabA, int64_t rowsU, int64_t ldA, const void* tabB, int64_t rowsI,
                              int64_t ldB, const NeumfGmf& g, const int64_t* idxU, const int64_t* idxI, int64_t B, int EA, int EB,
                              int n_layers, const int* dims, const void* packed, float* out, int32_t* oob, hipStream_t s) {
    if (!neumf_shape_ok(dtype, EA, EB, g.D, n_layers, dims))
        return fail(NCF_EUNSUPPORTED, "%s: no kernel for dtype=%d EA=%d EB=%d D=%d layers=%d", what, dtype, EA, EB, g.D, n_layers);
    if (B == 0) return NCF_OK;
    if (B < 0 || !tabA || !tabB || !packed || !out) return fail(NCF_EINVAL, "%s: bad argument", what);
    if (ldA < EA || ldB < EB || ldA % 4 || ldB % 4 || !aligned16(tabA) || !aligned16(tabB) || !aligned16(packed))
        return fail(NCF_EINVAL, "%s: tables must be 16-byte aligned with ld %% 4 == 0", what);
    if (const int rc = g.check(what, B, 1)) return rc;
    if (!idxU && B > rowsU) return fail(NCF_EINVAL, "%s: B = %lld > user table rows without user ids", what, (long long)B);
    if (!idxI && B > rowsI) return fail(NCF_EINVAL, "%s: B = %lld > item table rows without item ids", what, (long long)B);
    const BlobPtrs w = blob_ptrs(packed, dims, n_layers);
    NeumfArgs a;
    a.tabA = (const float*)tabA; a.rowsU = rowsU; a.ldA = ldA;
    a.tabB = (const float*)tabB; a.rowsI = rowsI; a.ldB = ldB;
    a.tabP = g.tabP; a.ldP = g.ldP; a.tabQ = g.tabQ; a.ldQ = g.ldQ;
    a.idxU = idxU; a.idxI = idxI; a.B = B; a.EA = EA; a.D = g.D;
    a.Wp1 = w.Wp1; a.b1 = w.b1; a.Wp2 = w.Wp2; a.b2 = w.b2; a.wl = w.wl; a.bl = w.bl;
    a.w = g.w; a.out = out; a.oob = oob;
    const int K0 = dims[0], N1 = dims[1], N2 = n_layers == 3 ? dims[2] : 0;
    const unsigned blocks = (unsigned)(((B + 31) / 32 + 3) / 4);
#define X(k0, n1, n2) \
    if (K0 == k0 && N1 == n1 && N2 == n2) hipLaunchKernelGGL((neumf_score_kernel<k0, n1, n2>), dim3(blocks), dim3(256), 0, s, a);
    NCF_FUSED_INSTANCES(X)
#undef X
    return check_launch(what);
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_neumf_supported(int dtype, int EA, int EB, int D, int n_layers, const int* dims) {
    return neumf_shape_ok(dtype, EA, EB, D, n_layers, dims) ? 1 : 0;
}

extern "C" int ncf_neumf_score(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB,
                               const float* gmfA, int64_t ldGA, const float* gmfB, int64_t ldGB, const int64_t* idxU, const int64_t* idxI,
                               int64_t B, int EA, int EB, int D, int n_layers, const int* dims, const void* packed, const float* w,
                               float* out, int32_t* oob, ncf_stream_t stream) {
    return neumf_score_launch("ncf_neumf_score", dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, NeumfGmf{gmfA, ldGA, gmfB, ldGB, D, w}, idxU,
                              idxI, B, EA, EB, n_layers, dims, packed, out, oob, (hipStream_t)stream);
}

extern "C" size_t ncf_neumf_topk_workspace_bytes(int64_t rows, int64_t cols, int n_layers, const int* dims, int D, int k) {
    if (!gmf_width_ok(D)) return 0;
    return mlp_topk_ws_bytes("ncf_neumf_topk_workspace_bytes", NeumfGmf{nullptr, 0, nullptr, 0, D, nullptr}, rows, cols, 1, n_layers, dims, k);
}

extern "C" int ncf_neumf_topk(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB,
                              const float* gmfA, int64_t ldGA, const float* gmfB, int64_t ldGB, int EA, int EB, int D,
                              const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims,
                              const void* packed, const float* w, const int64_t* seen_rowptr, const int32_t* seen_col, int k,
                              float* out_score, int32_t* out_idx, int32_t* out_count, void* workspace, size_t workspace_bytes, int32_t* oob,
                              ncf_stream_t stream) {
    return mlp_topk_run("ncf_neumf_topk", "ncf_neumf_topk_workspace_bytes", NeumfGmf{gmfA, ldGA, gmfB, ldGB, D, w}, dtype, tabA, rowsA, ldA,
                        tabB, rowsB, ldB, EA, EB, 1, user_ids, item_ids, rows, cols, n_layers, dims, packed, seen_rowptr, seen_col, k,
                        out_score, out_idx, out_count, workspace, workspace_bytes, oob, (hipStream_t)stream);
}

extern "C" size_t ncf_neumf_rank_workspace_bytes(int64_t rows, int64_t cols, int n_layers, const int* dims, int D, int64_t n_targets,
                                                 int max_targets) {
    if (!gmf_width_ok(D)) return 0;
    return mlp_rank_ws_bytes("ncf_neumf_rank_workspace_bytes", NeumfGmf{nullptr, 0, nullptr, 0, D, nullptr}, rows, cols, 1, n_layers, dims,
                             n_targets, max_targets);
}

extern "C" int ncf_neumf_rank(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB,
                              const float* gmfA, int64_t ldGA, const float* gmfB, int64_t ldGB, int EA, int EB, int D,
                              const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims,
                              const void* packed, const float* w, const int64_t* seen_rowptr, const int32_t* seen_col,
                              const int64_t* tgt_rowptr, const int32_t* tgt_col, int64_t n_targets, int max_targets, int32_t* rank,
                              int32_t* ranked, void* workspace, size_t workspace_bytes, int32_t* oob, int32_t* overflow,
                              ncf_stream_t stream) {
    const NeumfGmf g{gmfA, ldGA, gmfB, ldGB, D, w};
    hipStream_t s = (hipStream_t)stream;
    // the targets' own scores: the pair scorer over the (row, target) pairs
    auto score_pairs = [&](const int64_t* users, const int64_t* items, int64_t n, float* out) {
        return neumf_score_launch("ncf_neumf_rank", dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, g, users, items, n, EA, EB, n_layers, dims,
                                  packed, out, oob, s);
    };
    return mlp_rank_run("ncf_neumf_rank", "ncf_neumf_rank_workspace_bytes", g, score_pairs, dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, EA,
                        EB, 1, user_ids, item_ids, rows, cols, n_layers, dims, packed, seen_rowptr, seen_col, tgt_rowptr, tgt_col, n_targets,
                        max_targets, rank, ranked, workspace, workspace_bytes, oob, overflow, s);
}
