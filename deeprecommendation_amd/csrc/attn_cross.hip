// K3 cross-product form: AttentionNCF's attention of MANY users against ONE ranked list (full-catalogue top-K / ranks).
//
// The attention logit b1 + sum_a w1[a] relu(pc[i, a] + pr[e, a]) (and its cosine / linear forms) depends on the candidate item i
// and the rated item e only, never on the user.  When every user is scored against the same catalogue the logits are ONE
// (rated x candidate) table per weight version:
//   ncf_attn_logits   ST[e, i]  (transposed on purpose: for a fixed rated item, consecutive candidates are consecutive floats)
//   ncf_attn_cross    out[(u * I + j), :] = bias + sum_e softmax_e(ST[col_e, cand_j]) val_e feat[col_e, :]  per listed user u
// so per (user, candidate, entry) the work is a coalesced table lookup, one exponential and 2 * Fdim flops on the matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32), where the per-pair kernels of attn.hip recompute a 3 * A flop logit on the VALU.
#include "attn_util.h"

namespace ncf {

// ------------------------------------------------------------------------------------------------ the logit table
// One workgroup = a 64 x 64 tile of ST, thread (tx, ty) = 4 candidates x 4 rated items.  The operands are staged in chunks of 32
// hidden units; every logit is ONE fmaf chain over a = 0 .. A-1 in that order (then + b1), whatever the tile it falls in: the table is
// bitwise independent of the tiling.
constexpr int LG_T = 64, LG_AK = 32, LG_LD = LG_AK + 1;

template <int MODE>   // 0 MLP (max), 1 linear, 2 cosine, 3 MLP on the 2^-64-scaled operands (relu as the [0, 1] clamp)
__global__ __launch_bounds__(256) void attn_logits_kernel(const float* __restrict__ pc, int64_t ldpc, int64_t Ic,
                                                          const float* __restrict__ pr, int64_t ldpr, int64_t Ir, int A,
                                                          const float* __restrict__ w1, float b1, float* __restrict__ st, int64_t ldst) {
    __shared__ float pcs[LG_T * LG_LD], prs[LG_T * LG_LD], ws[LG_AK];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * LG_T, e0 = (int64_t)blockIdx.y * LG_T;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int a0 = 0; a0 < A; a0 += LG_AK) {
        const int na = A - a0 < LG_AK ? A - a0 : LG_AK;
        __syncthreads();
        for (int idx = t; idx < LG_T * LG_AK; idx += 256) {
            const int row = idx / LG_AK, a = idx % LG_AK;
            const bool in = a < na;
            pcs[row * LG_LD + a] = (in && i0 + row < Ic) ? pc[(i0 + row) * ldpc + a0 + a] : 0.f;
            prs[row * LG_LD + a] = (in && e0 + row < Ir) ? pr[(e0 + row) * ldpr + a0 + a] : 0.f;
        }
        if ((MODE == 0 || MODE == 3) && t < LG_AK) ws[t] = t < na ? w1[a0 + t] : 0.f;
        __syncthreads();
        for (int a = 0; a < na; ++a) {
            float cv[4], rv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) cv[c] = pcs[(4 * tx + c) * LG_LD + a];
#pragma unroll
            for (int r = 0; r < 4; ++r) rv[r] = prs[(4 * ty + r) * LG_LD + a];
            const float w = (MODE == 0 || MODE == 3) ? ws[a] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (MODE == 0) acc[r][c] = fmaf(w, fmaxf(cv[c] + rv[r], 0.f), acc[r][c]);
                    else if (MODE == 3) acc[r][c] = fmaf(w, __builtin_amdgcn_fmed3f(cv[c] + rv[r], 0.f, 1.f), acc[r][c]);
                    else if (MODE == 2) acc[r][c] = fmaf(cv[c], rv[r], acc[r][c]);
                    else acc[r][c] = cv[c] + rv[r];
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t e = e0 + 4 * ty + r;
        if (e >= Ir) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t i = i0 + 4 * tx + c;
            if (i < Ic) st[e * ldst + i] = acc[r][c] + ((MODE == 0 || MODE == 3) ? b1 : 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------ attention from the table
// One workgroup (4 waves) = (listed user, 128 candidates of the ranked list); a wave = 32 candidates.  Lane l of a wave is candidate
// l & 31 and entry parity h = l >> 5: exactly the A-operand map of the 32x32x2 MFMA (A[i = l & 31][k = l >> 5]).
//   pass 1  the lane walks the entries of its parity and keeps the maximum of ST[col_e, cand]; one exchange with the other parity.
//           The maximum is exact before any exponential is taken, so pass 2 needs no online rescale.
//   pass 2  tiles of TE entries: the tile's feat rows are staged once per workgroup in LDS (masked entries as zero rows); the lane
//           computes p = exp_le0(s - m) for its TE / 2 (candidate, entry) cells, adds them to l in entry order, and p * val is the A
//           operand, the LDS row the B operand (B[k = h][j = l & 31] = feat[col of entry 2 s + h][32 nb + j]) of one MFMA per
//           32-feature block nb: NB * 16 accumulators per lane.
//   final   out = acc / l + bias; l = 0 (empty / fully masked row, an all -inf table column, a refused index) gives the bias bits.
// No atomics; every sum has one fixed order (l: entry order per parity, then parity 0 + parity 1; the MFMA is a k-ordered fmaf
// chain), so the result is bitwise repeatable and independent of TE.
template <int NB, int TE>
__global__ __launch_bounds__(256) void attn_cross_kernel(const float* __restrict__ st, int64_t ldst, int64_t Ir, int64_t Ic,
                                                         const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, int64_t n_rows,
                                                         const int64_t* __restrict__ user_rows, const int64_t* __restrict__ cand_ids,
                                                         int64_t I, int64_t ntiles, const float* __restrict__ feat, int64_t ldfeat,
                                                         int fvec, const float* __restrict__ out_bias, float* __restrict__ out,
                                                         int64_t ldout, int32_t* __restrict__ oob) {
    constexpr int Fdim = NB * 32, KS = TE / 2;
    __shared__ __attribute__((aligned(16))) float fs[TE * Fdim];
    __shared__ int scol[TE];
    __shared__ float sval[TE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c32 = lane & 31, h = lane >> 5;
    const int64_t u = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int64_t row = user_rows[u];
    const bool row_ok = row >= 0 && row < n_rows;
    const int64_t jw = tile * 128 + wave * 32;                        // the wave's first column of the ranked list
    const int64_t j = jw + c32;
    int64_t cand = j < I ? (cand_ids ? cand_ids[j] : j) : 0;
    const bool cand_ok = cand >= 0 && cand < Ic;
    if (oob && (!row_ok || !cand_ok)) *oob = 1;                       // sticky; the pair's row is written as the bias
    if (!cand_ok) cand = 0;
    const bool live = row_ok && cand_ok && j < I;
    const int64_t beg = row_ok ? rowptr[row] : 0, end = row_ok ? rowptr[row + 1] : 0;
    const float* __restrict__ stc = st + cand;
    const bool wave_on = jw < I;                                      // wave-uniform

    // ---------------- pass 1: the exact row maximum ----------------
    float m = -INFINITY;
    if (live) {
        int64_t e = beg + h;
        for (; e + 6 < end; e += 8) {
            int cc[4];
            float sv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) cc[q] = col[e + 2 * q];
#pragma unroll
            for (int q = 0; q < 4; ++q) sv[q] = (cc[q] >= 0 && cc[q] < Ir) ? stc[(int64_t)cc[q] * ldst] : -INFINITY;
#pragma unroll
            for (int q = 0; q < 4; ++q) m = fmaxf(m, sv[q]);
        }
        for (; e < end; e += 2) {
            const int c = col[e];
            if (c >= 0 && c < Ir) m = fmaxf(m, stc[(int64_t)c * ldst]);
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32));
    const bool any = live && m != -INFINITY;

    // ---------------- pass 2: exponentials, their sum, the aggregation on the matrix cores ----------------
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    float l = 0.f;
    for (int64_t e0 = beg; e0 < end; e0 += TE) {
        __syncthreads();                                              // the previous tile has been read
        if (t < TE) {
            const int64_t e = e0 + t;
            const int c = e < end ? col[e] : -1;
            const bool ok = c >= 0 && c < Ir;
            scol[t] = ok ? c : -1;
            sval[t] = ok ? val[e] : 0.f;
        }
        if (fvec) {
            constexpr int F4 = Fdim / 4;
            for (int idx = t; idx < TE * F4; idx += 256) {
                const int r = idx / F4, f4 = idx % F4;
                const int64_t e = e0 + r;
                const int c = e < end ? col[e] : -1;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (c >= 0 && c < Ir) v = *reinterpret_cast<const f32x4*>(feat + (int64_t)c * ldfeat + 4 * f4);
                *reinterpret_cast<f32x4*>(fs + r * Fdim + 4 * f4) = v;
            }
        } else {
            for (int idx = t; idx < TE * Fdim; idx += 256) {
                const int r = idx / Fdim, f = idx % Fdim;
                const int64_t e = e0 + r;
                const int c = e < end ? col[e] : -1;
                fs[idx] = (c >= 0 && c < Ir) ? feat[(int64_t)c * ldfeat + f] : 0.f;
            }
        }
        __syncthreads();
        if (!wave_on) continue;                                       // wave-uniform: no barrier below
        float a[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = scol[2 * s + h];
            a[s] = (any && c >= 0) ? stc[(int64_t)c * ldst] : -INFINITY;
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float p = any ? exp_le0(a[s] - m) : 0.f;            // a masked entry: exp_le0(-inf) = 0
            l += p;
            a[s] = p * sval[2 * s + h];
        }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], fs[(2 * s + h) * Fdim + nb * 32 + c32], acc[nb], 0, 0, 0);
    }
    if (!wave_on) return;
    l = l + __shfl_xor(l, 32);                                        // both parities hold parity 0 + parity 1 (commutative: same bits)
    const float inv = l > 0.f ? 1.0f / l : 0.f;

    // ---------------- final: lane = feature 32 nb + c32, register r = candidate acc_row(r, h) of the wave ----------------
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cr = acc_row(r, h);
        const float invr = __shfl(inv, cr);
        const int64_t jr = jw + cr;
        if (jr >= I) continue;
        float* __restrict__ o = out + (u * I + jr) * ldout;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float b = out_bias ? out_bias[nb * 32 + c32] : 0.f;
            o[nb * 32 + c32] = invr > 0.f ? fmaf(acc[nb][r], invr, b) : b;
        }
    }
}

struct AttnCrossPlan {
    int status, nb, te;
    int64_t lds, grid;
    const char* why;
};

static AttnCrossPlan plan_attn_cross(int Fdim, int64_t U, int64_t I) {
    AttnCrossPlan p{NCF_OK, 0, 0, 0, 0, ""};
    if (Fdim % 32 != 0 || Fdim < 32 || Fdim > 256) {
        p.status = NCF_EUNSUPPORTED;
        p.why = "Fdim must be a multiple of 32 in 32 .. 256";
        return p;
    }
    if (U < 0 || I < 0) {
        p.status = NCF_EINVAL;
        p.why = "bad sizes";
        return p;
    }
    p.nb = Fdim / 32;
    p.te = p.nb <= 4 ? 64 : 32;                                       // the staged tile stays within 32 KiB of static LDS
    p.lds = (int64_t)p.te * Fdim * 4 + p.te * 8;
    const int64_t ntiles = (I + 127) / 128;
    if (U > 0 && ntiles > 0 && ntiles > (int64_t)0x7FFFFFFF / U) {
        p.status = NCF_EUNSUPPORTED;
        p.why = "more than 2^31 - 1 workgroups";
        return p;
    }
    p.grid = U * ntiles;
    return p;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_attn_logits(int mode, const float* pc, int64_t ldpc, int64_t Ic, const float* pr, int64_t ldpr, int64_t Ir, int A,
                               const float* w1, float b1, float* st, int64_t ldst, ncf_stream_t stream) {
    if (mode < 0 || mode > 3) return fail(NCF_EINVAL, "ncf_attn_logits: bad mode %d", mode);
    if (Ic < 0 || Ir < 0 || A <= 0) return fail(NCF_EINVAL, "ncf_attn_logits: bad sizes");
    if (Ic == 0 || Ir == 0) return NCF_OK;
    if (!pc || !pr || !st) return fail(NCF_EINVAL, "ncf_attn_logits: null pointer");
    if ((mode == NCF_ATT_MLP || mode == NCF_ATT_MLP_SCALED) && !w1) return fail(NCF_EINVAL, "ncf_attn_logits: w1 is null");
    if (mode == NCF_ATT_LINEAR && A != 1) return fail(NCF_EINVAL, "ncf_attn_logits: linear mode needs A == 1");
    if (ldpc < A || ldpr < A || ldst < Ic) return fail(NCF_EINVAL, "ncf_attn_logits: leading dimension smaller than row");
    const int64_t gx = (Ic + LG_T - 1) / LG_T, gy = (Ir + LG_T - 1) / LG_T;
    if (gx > 0x7FFFFFFF || gy > 65535) return fail(NCF_EUNSUPPORTED, "ncf_attn_logits: more than 65535 x 64 rated items");
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(M) hipLaunchKernelGGL((attn_logits_kernel<M>), grid, dim3(256), 0, s, pc, ldpc, Ic, pr, ldpr, Ir, A, w1, b1, st, ldst)
    if (mode == 0) LAUNCH(0);
    else if (mode == 1) LAUNCH(1);
    else if (mode == 2) LAUNCH(2);
    else LAUNCH(3);
#undef LAUNCH
    return check_launch("ncf_attn_logits");
}

extern "C" int ncf_attn_cross_supported(int Fdim) {
    return (Fdim % 32 == 0 && Fdim >= 32 && Fdim <= 256) ? 1 : NCF_EUNSUPPORTED;
}

extern "C" int ncf_attn_cross_plan(int Fdim, int64_t U, int64_t I, int* nb, int* entry_tile, int64_t* lds_bytes, int64_t* grid_x) {
    const AttnCrossPlan p = plan_attn_cross(Fdim, U, I);
    if (p.status != NCF_OK) return fail(p.status, "ncf_attn_cross_plan: %s (Fdim = %d)", p.why, Fdim);
    if (nb) *nb = p.nb;
    if (entry_tile) *entry_tile = p.te;
    if (lds_bytes) *lds_bytes = p.lds;
    if (grid_x) *grid_x = p.grid;
    return NCF_OK;
}

extern "C" int ncf_attn_cross(const float* st, int64_t ldst, int64_t Ir, int64_t Ic, const int64_t* rowptr, const int32_t* col,
                              const float* val, int64_t n_rows, const int64_t* user_rows, int64_t U, const int64_t* cand_ids,
                              int64_t I, const float* feat, int64_t ldfeat, int Fdim, const float* out_bias, float* out,
                              int64_t ldout, int32_t* oob, ncf_stream_t stream) {
    const AttnCrossPlan p = plan_attn_cross(Fdim, U, I);
    if (p.status != NCF_OK) return fail(p.status, "ncf_attn_cross: %s (Fdim = %d)", p.why, Fdim);
    if (Ir < 0 || Ic < 0 || n_rows < 0) return fail(NCF_EINVAL, "ncf_attn_cross: bad sizes");
    if (U == 0 || I == 0) return NCF_OK;
    if (!st || !rowptr || !user_rows || !feat || !out) return fail(NCF_EINVAL, "ncf_attn_cross: null pointer");
    if (ldst < Ic || ldfeat < Fdim || ldout < Fdim) return fail(NCF_EINVAL, "ncf_attn_cross: leading dimension smaller than row");
    if (!cand_ids && I > Ic) return fail(NCF_EINVAL, "ncf_attn_cross: I = %lld > I_c = %lld without dev_cand_ids", (long long)I, (long long)Ic);
    const int fvec = aligned16(feat) && ldfeat % 4 == 0;
    const int64_t ntiles = (I + 127) / 128;
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(N, T)                                                                                                             \
    hipLaunchKernelGGL((attn_cross_kernel<N, T>), dim3((unsigned)p.grid), dim3(256), 0, s, st, ldst, Ir, Ic, rowptr, col, val, n_rows, \
                       user_rows, cand_ids, I, ntiles, feat, ldfeat, fvec, out_bias, out, ldout, oob)
    switch (p.nb) {
        case 1: LAUNCH(1, 64); break;
        case 2: LAUNCH(2, 64); break;
        case 3: LAUNCH(3, 64); break;
        case 4: LAUNCH(4, 64); break;
        case 5: LAUNCH(5, 32); break;
        case 6: LAUNCH(6, 32); break;
        case 7: LAUNCH(7, 32); break;
        default: LAUNCH(8, 32); break;
    }
#undef LAUNCH
    return check_launch("ncf_attn_cross");
}
