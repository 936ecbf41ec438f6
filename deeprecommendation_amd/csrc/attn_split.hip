// K3 grouped, ENTRY-SPLIT form (round 3): AttentionNCF item-item attention (models/attention_ncf.py:154-216, eval mode) for pairs
// that share rated sets, fp32, gfx950.
//
// The scalar-operand grouped kernel (attn.hip, round 2) gives one workgroup up to 32 pairs of ONE user and walks the user's whole
// rated set tile by tile: a batch of 4096 pairs is 1024 four-pair wave jobs — one wave per SIMD on the chip — each a serial chain
// of 4 tiles x (DMA wait, 3 barriers, ~1400 instructions), at 256 VGPRs with 22 of them spilled to scratch.  Measured 36 us where
// the arithmetic is a few us of the chip: the kernel is bound by its own critical path, not by a unit.
// Here the unit of work is (group of pairs) x (a SLICE of the rated set): gridDim.y = nsplit slices, each workgroup runs the same
// tile pipeline over its tiles only and leaves a softmax PARTIAL per pair — running maximum m, sum l and the un-normalised
// aggregate O (Fdim floats) — which attn_combine_kernel merges:  out = sum_s O_s e^(m_s - M) / sum_s l_s e^(m_s - M) + bias.
// Four times the workgroups at a quarter of the chain; and the kernel is built for <= 128 VGPRs (row blocks of 8 chunks, double
// buffered, instead of the lane's whole 128-float row), so two 512-thread workgroups share a CU — four waves per SIMD cover each
// other's scalar-load, LDS and DMA latencies.  No spills: the arguments travel as one struct (read on demand from the kernarg
// segment), the workgroup -> row map is an array written by the grouping pass (the binary search over wg_ptr was 6 dependent
// global loads before the first useful instruction), and nothing zero-fills LDS (masked entries gather row 0 and weigh 0).
//   * lane = entry of the 64-entry tile; a wave scores its 4 pairs against the lane's row block with pc rows and w1 as SCALAR
//     operands of packed fp32 ops (s_load -> SGPR pairs; relu = the clamp modifier of the packed add on 2^-64-scaled operands);
//   * tiles arrive by LDS-DMA (global_load_lds_dwordx4, source-swizzled for conflict-free row reads);
//   * the aggregation over the tile's entries runs on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 fmaf chains).
// Same arithmetic per (pair, entry) as the round-2 kernel; the split only changes where the softmax partials are merged, i.e. the
// fp32 summation order (held to 1e-5 against the per-pair kernel and the oracle).  Fixed split: bitwise reproducible run to run.
#include "ncf_common.h"
#include "attn_tile.h"
#include <math.h>
#include <atomic>
#include <type_traits>

namespace ncf {

struct AttnSplitArgs {
    const float* pc; const float* pr; const float* w1; const float* feat; const float* out_bias;
    const int64_t* rowptr; const int32_t* col; const float* val;
    const int64_t* grp_ptr; const int64_t* pair_ids; const int64_t* wg_ptr; const int32_t* wg_row;
    float* out; float* part;
    int64_t R, I;
    int ldpc, ldpr, ldfeat, ldout, A, Fdim, ppw, nsplit, ldpart;
    float b1;
};

// MODE 0: MLP (relu + w1 dot), 2: cosine (dot of normalised rows), 3: MLP on 2^-64-scaled operands (relu = clamp)
// NW = 4 / 8 / 16 waves x 4 pairs (a user's pairs share the staged tile: 64 pairs per workgroup halve the gathered bytes per pair of
// 32, and a (user, tile) unit of a 64-pairs-per-user batch is ONE workgroup per CU instead of two or three); FD = Fdim (compile-time: the aggregation's B-operand reads walk the feat image with a stride of Fdim floats —
// with a run-time stride hipcc keeps 16 precomputed addresses per lane, and spills them)
// The stages are attn_tile.h's.  pc rows and w1 travel through the CONSTANT address space (LoadConst: the arguments are a by-value
// struct), one 16-byte chunk per pair (+ w1's) per scalar-load step: 20 SGPRs per step and buffer.
template <int MODE, int NW, int FD>
__global__ __launch_bounds__(64 * NW, 4) void attn_split_kernel(const AttnSplitArgs a) {
    constexpr int EC = kTileEC, MAXP = kTileMaxP, PP = MAXP * NW, MT = PP / 16, PS = kTilePS, CB = 8;
    constexpr int Fdim = FD, F4 = FD / 4, NTILES = FD / 16, NJ = (MT * NTILES + NW - 1) / NW;   // NJ = 16x16 aggregation tiles per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int A = a.A, A4 = A >> 2;
    const AttnTileLds lay = attn_tile_lds(A, Fdim, PP);
    float* prt = reinterpret_cast<float*>(smem) + lay.prt;
    float* fct = reinterpret_cast<float*>(smem) + lay.fct;
    float* Pm = reinterpret_cast<float*>(smem) + lay.Pm;
    float* scl = reinterpret_cast<float*>(smem) + lay.scl;
    int64_t* pid = reinterpret_cast<int64_t*>(reinterpret_cast<float*>(smem) + lay.pid);
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t g = blockIdx.x;
    const int split = blockIdx.y;
    if (g >= a.wg_ptr[a.R]) return;                        // the grid is an upper bound (no host sync for its size)
    const AttnGroup grp = attn_group_lookup(g, a.wg_ptr, a.grp_ptr, a.R, a.ppw, a.wg_row);   // wg_row: written by the grouping pass
    const int64_t r = grp.r, start = grp.start;
    const int cnt = grp.cnt;
    const int64_t rbeg = a.rowptr[r], rend = a.rowptr[r + 1];
    // this workgroup's slice of the row's tiles
    const int64_t row_tiles = (rend - rbeg + EC - 1) / EC;
    const int64_t t0 = split * row_tiles / a.nsplit, t1 = (split + 1) * row_tiles / a.nsplit;
    const int64_t beg = rbeg + t0 * EC;
    const int64_t end = rbeg + t1 * EC < rend ? rbeg + t1 * EC : rend;
    const int64_t ntiles = t1 - t0;

    // the wave's pairs: slots j = wave + NW*k; their pc rows are wave-uniform pointers (scalar loads)
    const int np = cnt > wave ? (cnt - wave + NW - 1) / NW : 0;
    const float* pcrow[MAXP];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
        const int j = k < np ? wave + NW * k : 0;
        pcrow[k] = a.pc + uniform64(a.pair_ids[start + j]) * a.ldpc;
    }
    if (tid < PP) pid[tid] = tid < cnt ? a.pair_ids[start + tid] : -1;

    const bool swz = (A4 % 16) == 0;
    const int shA = (A4 & (A4 - 1)) == 0 ? __builtin_ctz(A4) : -1;
    constexpr int shF = (F4 & (F4 - 1)) == 0 ? __builtin_ctz(F4) : -1;
    // nothing zero-fills LDS: a masked entry (outside the slice / the catalogue) gathers row 0 and weighs 0
    const TileEntries<decltype(a.col), decltype(a.val)> ent{a.col, a.val, beg, end, a.I, lane};
    auto issue_pr = [&](int cols) { tile_issue<true, NW>(a.pr, a.ldpr, A4, shA, swz, lds0, cols, lane, wave); };
    auto issue_feat = [&](int cols) { tile_issue<true, NW>(a.feat, a.ldfeat, F4, shF, false, lds0 + (unsigned)(EC * A * 4), cols, lane, wave); };

    f32x4 acc[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[MAXP], l[MAXP];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) { m[k] = -INFINITY; l[k] = 0.f; }

    int c_cur = -1, c_nxt = -1;
    float v_cur = 0.f, v_nxt = 0.f;
    if (ntiles > 0) {
        ent.load(beg, c_cur, v_cur);
        ent.load(beg + EC, c_nxt, v_nxt);
        c_cur = ent.valid(beg, c_cur);
        c_nxt = ent.valid(beg + EC, c_nxt);
        issue_pr(c_cur);
        issue_feat(c_cur);
    }
    const int sw = swz ? (lane & 15) : 0;
    const int g4 = lane >> 4, i16 = lane & 15;
    const float* myrow = prt + lane * A;
    const int NB = A4 / CB;
    for (int64_t t = 0; t < ntiles; ++t) {
        const int64_t e0 = beg + t * EC;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of pr(t) / feat(t) have landed (and col / val) ...
        __syncthreads();                                   // ... and everybody's; pid is written
        const bool ok = c_cur >= 0;
        const float vl = ok ? v_cur : 0.f;
        int c_nn = -1;
        float v_nn = 0.f;
        if (t + 2 < ntiles) ent.load(e0 + 2 * EC, c_nn, v_nn);   // wave-uniform

        f32x2 s2[MAXP], t2[MAXP];
#pragma unroll
        for (int k = 0; k < MAXP; ++k) { s2[k] = f32x2{0.f, 0.f}; t2[k] = f32x2{0.f, 0.f}; }
        // Row blocks of CB chunks, one at a time: four waves per SIMD cover a block's LDS reads.  (Double buffering the blocks in
        // registers spills at the 128-register budget, and touching the next block's pc / w1 lines ahead measured slower: DESIGN.md.)
        for (int blk = 0; blk < NB; ++blk) {
            f32x4 rA[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) rA[c] = *reinterpret_cast<const f32x4*>(myrow + 4 * ((blk * CB + c) ^ sw));
            tile_score<MODE, 1, CB>(np, rA, a.w1, pcrow, blk * CB, s2, t2, LoadConst{});
        }
        float sc[MAXP], mx[MAXP];
        tile_scores<MODE>(s2, t2, ok, a.b1, sc, mx);
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            const SoftmaxStep st = tile_softmax_step(m[k], l[k], mx[k], sc[k], ok && k < np);
            const int j = wave + NW * k;                   // every slot of the wave writes (slots beyond np: zeros) — nothing
            Pm[j * PS + lane] = st.pe * vl;                // uninitialised ever reaches an MFMA
            if (lane == 0) scl[j] = (k < np) ? st.scale : 0.f;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // P and scl of this tile are complete; every wave is done with the pr image
        if (t + 1 < ntiles) issue_pr(c_nxt);               // tile t+1's rows land under this tile's aggregation
        tile_aggregate<NW, MT, NJ>(acc, fct, Pm, scl, Fdim, NTILES, wave, g4, i16);
        if (t + 1 < ntiles) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of the feat image / P have returned
            __builtin_amdgcn_s_barrier();
            c_cur = c_nxt; v_cur = v_nxt;
            c_nxt = ent.valid(e0 + 2 * EC, c_nn); v_nxt = v_nn;
            issue_feat(c_cur);
        }
    }
    // ---- the slice's softmax partials (nsplit > 1) or the finished rows (nsplit == 1) ----
    float lt[MAXP];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) lt[k] = l[k];
    wave_reduce_dpp_n<MAXP>(lt, [](float x, float y) { return x + y; });
    __syncthreads();                                       // the last tile's MFMAs have read scl; pid is visible (also when ntiles == 0)
    if (a.nsplit > 1) {
#pragma unroll
        for (int k = 0; k < MAXP; ++k)
            if (k < np && lane == 0) {
                float* ph = a.part + (pid[wave + NW * k] * a.nsplit + split) * (int64_t)a.ldpart;
                ph[0] = m[k];
                ph[1] = lt[k];
            }
#pragma unroll
        for (int n = 0; n < NJ; ++n) {
            const int job = wave + NW * n;
            const int mt = job % MT, nt = job / MT;
            if (nt >= NTILES) break;
            const int f = 16 * nt + i16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * mt + 4 * g4 + i;
                if (row < cnt && f < Fdim) a.part[(pid[row] * a.nsplit + split) * (int64_t)a.ldpart + kPartHead + f] = acc[n][i];
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < MAXP; ++k)
        if (lane == 0) scl[wave + NW * k] = (k < np && lt[k] > 0.f) ? 1.0f / lt[k] : 0.f;
    __syncthreads();
    tile_store_scaled<NW, MT, NJ>(acc, scl, pid, cnt, Fdim, NTILES, a.out_bias, a.out, a.ldout, wave, g4, i16);
}

// out[b, :] = the merge of pair b's slice partials + bias (merge_partials, attn_tile.h), four features per thread
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ part, int ldpart, int nsplit, int64_t B, int Fdim,
                                                           const float* __restrict__ out_bias, float* __restrict__ out, int64_t ldout) {
    const int F4 = Fdim >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * F4) return;
    const int64_t b = i / F4;
    const int c = (int)(i - b * F4);
    const f32x4 o = merge_partials<false>(part + b * nsplit * (int64_t)ldpart, nsplit, ldpart, c, out_bias);
    float* dst = out + b * ldout + 4 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = o[j];
}

}  // namespace ncf

using namespace ncf;

extern "C" size_t ncf_attn_split_workspace_bytes(int64_t B, int Fdim, int nsplit) {
    if (B <= 0 || Fdim <= 0 || nsplit <= 1) return 0;
    return (size_t)B * (size_t)nsplit * (size_t)(Fdim + kPartHead) * sizeof(float);
}

extern "C" int ncf_attn_split_supported(int mode, int A, int Fdim, int pairs_per_wg) {
    if (mode != NCF_ATT_MLP && mode != NCF_ATT_COS && mode != NCF_ATT_MLP_SCALED) return 0;
    if (A <= 0 || A % 32 || A > 256 || (Fdim != 64 && Fdim != 128)) return 0;
    if (pairs_per_wg < 1 || pairs_per_wg > 64) return 0;
    return attn_tile_lds(A, Fdim, attn_tile_pairs(pairs_per_wg)).bytes() <= 160 * 1024;
}

extern "C" int ncf_attn_forward_split(int mode, const float* pc, int64_t ldpc, const float* pr, int64_t ldpr, int A, const float* w1,
                                      float b1, const int64_t* rowptr, const int32_t* col, const float* val, int64_t R, int64_t I,
                                      const int64_t* grp_ptr, const int64_t* pair_ids, const int64_t* wg_ptr, const int32_t* wg_row,
                                      int64_t B, int pairs_per_wg, const float* feat, int64_t ldfeat, int Fdim, const float* out_bias,
                                      float* out, int64_t ldout, int nsplit, int merge, void* workspace, size_t workspace_bytes,
                                      ncf_stream_t stream) {
    if (!ncf_attn_split_supported(mode, A, Fdim, pairs_per_wg))
        return fail(NCF_EUNSUPPORTED, "ncf_attn_forward_split: needs MLP / cosine mode, A %% 32 == 0 and <= 256, Fdim 64 or 128 (A = %d, Fdim = %d)", A, Fdim);
    if (B < 0 || R < 0 || I < 0 || nsplit < 1 || nsplit > 64) return fail(NCF_EINVAL, "ncf_attn_forward_split: bad sizes");
    if (B == 0 || R == 0) return NCF_OK;
    if (I == 0) return fail(NCF_EINVAL, "ncf_attn_forward_split: empty catalogue with non-empty rows");
    if (!pc || !pr || !rowptr || !col || !val || !grp_ptr || !pair_ids || !wg_ptr || !feat || !out)
        return fail(NCF_EINVAL, "ncf_attn_forward_split: null pointer");
    if (mode != NCF_ATT_COS && !w1) return fail(NCF_EINVAL, "ncf_attn_forward_split: w1 is null");
    if (ldpc < A || ldpr < A || ldfeat < Fdim || ldout < Fdim) return fail(NCF_EINVAL, "ncf_attn_forward_split: leading dimension smaller than row");
    if (ldpc % 4 || ldpr % 4 || ldfeat % 4 || ldpc >= (1ll << 31) || ldpr >= (1ll << 31) || ldfeat >= (1ll << 31) || ldout >= (1ll << 31))
        return fail(NCF_EUNSUPPORTED, "ncf_attn_forward_split: leading dimensions must be multiples of 4 below 2^31");
    if (!aligned16(pc) || !aligned16(pr) || (w1 && !aligned16(w1)) || !aligned16(feat) || (out_bias && !aligned16(out_bias)))
        return fail(NCF_EINVAL, "ncf_attn_forward_split: operands must be 16-byte aligned");
    if (nsplit > 1 && (!workspace || workspace_bytes < ncf_attn_split_workspace_bytes(B, Fdim, nsplit) || !aligned16(workspace)))
        return fail(NCF_EWORKSPACE, "ncf_attn_forward_split: workspace too small (ncf_attn_split_workspace_bytes) or misaligned");
    hipStream_t s = (hipStream_t)stream;
    AttnSplitArgs a;
    a.pc = pc; a.pr = pr; a.w1 = w1; a.feat = feat; a.out_bias = out_bias;
    a.rowptr = rowptr; a.col = col; a.val = val; a.grp_ptr = grp_ptr; a.pair_ids = pair_ids; a.wg_ptr = wg_ptr; a.wg_row = wg_row;
    a.out = out; a.part = (float*)workspace;
    a.R = R; a.I = I;
    a.ldpc = (int)ldpc; a.ldpr = (int)ldpr; a.ldfeat = (int)ldfeat; a.ldout = (int)ldout; a.A = A; a.Fdim = Fdim;
    a.ppw = pairs_per_wg; a.nsplit = nsplit; a.ldpart = Fdim + kPartHead;
    a.b1 = b1;
    const unsigned blocks = (unsigned)((B + pairs_per_wg - 1) / pairs_per_wg + (R < B ? R : B));   // upper bound on sum_r ceil(n_r / ppw)
    const int pp = attn_tile_pairs(pairs_per_wg);   // 4 / 8 / 16 waves of 4 pairs
    const size_t lds = attn_tile_lds(A, Fdim, pp).bytes();
    const bool scaled = mode == NCF_ATT_MLP_SCALED;
#define LAUNCH_SP(M, W, J)                                                                                              \
    do {                                                                                                                \
        static std::atomic<unsigned long long> done{0};                                                                 \
        if (lds > 64 * 1024 && !raise_lds((const void*)attn_split_kernel<M, W, J>, done))                               \
            return fail(NCF_EUNSUPPORTED, "ncf_attn_forward_split: cannot reserve %zu bytes of LDS", lds);               \
        hipLaunchKernelGGL((attn_split_kernel<M, W, J>), dim3(blocks, (unsigned)nsplit), dim3(64 * W), lds, s, a);        \
    } while (0)
#define LAUNCH_SP_J(M, W) do { if (Fdim == 64) LAUNCH_SP(M, W, 64); else LAUNCH_SP(M, W, 128); } while (0)
#define LAUNCH_SP_W(M) do { if (pp == 16) LAUNCH_SP_J(M, 4); else if (pp == 32) LAUNCH_SP_J(M, 8); else LAUNCH_SP_J(M, 16); } while (0)
    if (mode == NCF_ATT_COS) LAUNCH_SP_W(2);
    else if (scaled) LAUNCH_SP_W(3);
    else LAUNCH_SP_W(0);
#undef LAUNCH_SP_W
#undef LAUNCH_SP_J
#undef LAUNCH_SP
    int rc = check_launch("ncf_attn_forward_split");
    if (rc != NCF_OK || nsplit == 1 || !merge) return rc;   // merge == 0: the partials stay in the workspace (ncf_attn_tail merges them)
    const int64_t n = B * (Fdim / 4);
    hipLaunchKernelGGL(attn_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)workspace, Fdim + kPartHead, nsplit, B,
                       Fdim, out_bias, out, ldout);
    return check_launch("ncf_attn_forward_split (combine)");
}
