// The stages of the tiled grouped attention kernels, one copy each: attn_grouped_sc_kernel (attn.hip, scalar-operand form) and
// attn_split_kernel (attn_split.hip, entry-split form) run the same tile pipeline — a workgroup takes up to ppw pairs of one rated
// set, lane = entry of a 64-entry tile, a wave scores its 4 pairs against the lane's pr row with pc rows and w1 as scalar operands,
// tiles arrive by LDS-DMA, the aggregation runs on the matrix cores — and differ in what they walk (the whole row / a slice of it),
// in how they order the stages around their barriers, and in what they leave (finished rows / softmax partials).  The stages below
// are what the two hold in common; the order of the stages, the barriers and the waits stay in the kernels.  Also here: the LDS
// layout both launch sites size, the workgroup -> row lookup (attn_grouped_kernel takes it too), and the merge of the split form's
// partials (attn_combine_kernel and attn_tail_kernel).  Everything is forced inline.  The group lookup and the entry loads take
// their operands by REFERENCE, as the lambdas they replace captured them: an operand that is a field of a by-value kernel argument
// struct is then read from the kernarg segment where the stage uses it, not where the stage is called — with that the entry
// loads leave both kernels' listings as they were; the other stages take values (compared both ways).  One stage is NOT taken
// from here by attn_grouped_sc_kernel: its score step stays written out in attn.hip, where it measured faster.
// Internal.
#pragma once
#include "attn_util.h"

namespace ncf {

constexpr int kTileEC = 64;     // entries per tile = lanes
constexpr int kTileMaxP = 4;    // pairs (slots) per wave
constexpr int kTilePS = 66;     // row stride of the P image, floats
constexpr int kPartHead = 4;    // floats in front of a partial's O: m, l, (2 unused: O stays 16-byte aligned)

// ---- LDS layout: [EC][A] pr tile image (DMA) | [EC][Fdim] feat tile image (DMA) | [pp][PS] p_e * val_e of the current tile, pair-major |
// [pp] the tile's rescale factor per pair | [pp] int64 output row of each pair.  pp = pairs_per_wg rounded to 4 / 8 / 16 waves of 4 pairs.
struct AttnTileLds {
    int prt, fct, Pm, scl, pid;   // offsets in floats
    int floats;
    __host__ __device__ constexpr size_t bytes() const { return (size_t)floats * 4; }
};
__host__ __device__ constexpr int attn_tile_pairs(int pairs_per_wg) { return pairs_per_wg <= 16 ? 16 : (pairs_per_wg <= 32 ? 32 : 64); }
__host__ __device__ constexpr AttnTileLds attn_tile_lds(int A, int Fdim, int pp) {
    return {0, kTileEC * A, kTileEC * A + kTileEC * Fdim, kTileEC * A + kTileEC * Fdim + pp * kTilePS, kTileEC * A + kTileEC * Fdim + pp * kTilePS + pp,
            kTileEC * (A + Fdim) + pp * kTilePS + pp + 2 * pp};
}

// ---- workgroup g -> its row r (wg_ptr[r] <= g < wg_ptr[r+1]: read from wg_row when the grouping pass wrote it, else searched), the
// first of its pairs in pair_ids and their number.  The caller has left if g >= wg_ptr[R] (the grid is an upper bound: no host sync
// for its size).
struct AttnGroup {
    int64_t r, start;
    int cnt;
};
template <typename P64, typename P32>   // const int64_t* / const int32_t*, __restrict__ or not
__device__ __forceinline__ AttnGroup attn_group_lookup(const int64_t& g, const P64& wg_ptr, const P64& grp_ptr, const int64_t& R, const int& ppw,
                                                       const P32& wg_row) {
    int64_t r;
    if (wg_row) {
        r = wg_row[g];
    } else {
        int64_t lo = 0, hi = R;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (wg_ptr[mid] <= g) lo = mid; else hi = mid;
        }
        r = lo;
    }
    const int64_t start = grp_ptr[r] + (g - wg_ptr[r]) * ppw;
    const int64_t left = grp_ptr[r + 1] - start;
    return {r, start, (int)(left < ppw ? left : ppw)};
}

// ---- the tile's own entry of this lane: column and rating, loaded ahead of their use — unconditionally (index clamped into
// [beg, end)) and back to back: a dependent load would need a vmcnt wait, and every vmcnt wait also drains the tile DMAs in flight.
// Validity (inside the range, column inside the catalogue) is decided when the values are used.
template <typename PC, typename PV>        // const int32_t* / const float*, __restrict__ or not
struct TileEntries {
    const PC& col;
    const PV& val;
    const int64_t &beg, &end, &I;
    const int& lane;
    __device__ __forceinline__ void load(int64_t e0, int& c, float& v) const {
        const int64_t e = e0 + lane < end ? e0 + lane : (end > beg ? end - 1 : beg);
        c = end > beg ? col[e] : -1;
        v = end > beg ? val[e] : 0.f;
    }
    __device__ __forceinline__ int valid(int64_t e0, int c) const { return (e0 + lane < end && c >= 0 && c < I) ? c : -1; }
};

// ---- LDS-DMA of one image of a tile: EC rows of X4 16-byte chunks = X4 pieces (one wave-instruction, 64 chunks, 1 KiB); wave w
// issues pieces w, w + NW, ...  `cols` = this lane's col of the tile being fetched (or -1: masked).  A piece's lane writes chunk j
// of entry e and fetches SOURCE chunk j ^ (e & 15) when xorj (rows that are whole 256-byte bank rows: the reader applies the same
// XOR).  A piece covers 64 / X4 whole rows when rows are a power of two of chunks (shX = log2 X4, else -1): the row's col then
// comes from 1 / 2 / 4 readlanes (no LDS round trip, nothing to wait for) and every piece costs a dozen instructions.
// ROW0: a masked entry gathers row 0 (and weighs 0); else its DMA is skipped (the caller's LDS holds zeros there).
template <bool ROW0, int NW>
__device__ __forceinline__ void tile_issue(const float* tab, int64_t ld, int X4, int shX, bool xorj, unsigned lds_base, int cols, int lane, int wave) {
    const int rpp = shX >= 0 ? 64 >> shX : 0;
    if (rpp >= 1 && rpp <= 4) {
        const int sub = lane >> shX, j = lane & (X4 - 1);
        for (int piece = wave; piece < X4; piece += NW) {   // wave-uniform trip count
            const int e0p = piece * rpp;
            int ci = __builtin_amdgcn_readlane(cols, e0p);
            if (rpp >= 2) { const int c1 = __builtin_amdgcn_readlane(cols, e0p + 1); ci = sub == 1 ? c1 : ci; }
            if (rpp == 4) {
                const int c2 = __builtin_amdgcn_readlane(cols, e0p + 2), c3 = __builtin_amdgcn_readlane(cols, e0p + 3);
                ci = sub == 2 ? c2 : (sub == 3 ? c3 : ci);
            }
            const int jj = xorj ? (j ^ ((e0p + sub) & 15)) : j;
            if (ROW0 || ci >= 0) dma16(tab + (int64_t)(ROW0 ? (ci >= 0 ? ci : 0) : ci) * ld + 4 * jj, lds_base + (unsigned)piece * 1024u);
        }
        return;
    }
    for (int piece = wave; piece < X4; piece += NW) {  // general row widths: (entry, chunk) by division, col by a shuffle
        const int gi = piece * 64 + lane;
        const int e = shX >= 0 ? gi >> shX : gi / X4;
        const int j = shX >= 0 ? gi & (X4 - 1) : gi - e * X4;
        const int ci = __shfl(cols, e);
        if (ROW0 || ci >= 0)
            dma16(tab + (int64_t)(ROW0 ? (ci >= 0 ? ci : 0) : ci) * ld + 4 * (xorj ? (j ^ (e & 15)) : j), lds_base + (unsigned)piece * 1024u);
    }
}

// ---- the operand load form of the score step.  pc rows and w1 are read-only for the whole launch and wave-uniform.  Through a
// pointer of a by-value argument struct hipcc cannot prove the memory invariant and emits vector loads unless the pointer is in
// the CONSTANT address space (LoadConst: s_load_dwordx4).  attn_grouped_sc_kernel reads them through its __restrict__ arguments
// as they are; its score step is the one stage that stays written out in the kernel (called from here it measured slower).
typedef const f32x4 __attribute__((address_space(4))) * const_f32x4_ptr;
struct LoadConst {
    __device__ __forceinline__ f32x4 operator()(const float* p) const { return *(const_f32x4_ptr)(p); }
};

// ---- scores of NS slots (1, 2 or 4, >= the wave's pairs) against CB chunks of the lane's row, chunks c0 .. c0 + CB - 1 of the rows.
// MODE 0: MLP (relu + w1 dot), 2: cosine (dot of normalised rows), 3: MLP on 2^-64-scaled operands.
// Scalar operands arrive G chunks per pair (+ w1's) at a time, one step ahead: a wait on scalar loads is always lgkmcnt(0) (they
// return out of order), so the order inside a step is  wait(step s) -> issue loads(step s+1) -> VALU(step s): the next step's
// loads fly under this step's arithmetic, and the live scalars stay at two steps' worth (all of them at once would be 1024 SGPRs:
// spilled through v_writelane / v_readlane).
template <int MODE, int NS, int G, int CB, typename Load>
__device__ __forceinline__ void tile_score_block(const f32x4 (&row)[CB], const float* w1, const float* (&pcrow)[kTileMaxP], int c0,
                                                 f32x2 (&s2)[kTileMaxP], f32x2 (&t2)[kTileMaxP], Load ld) {
    constexpr int NST = CB / G;
    f32x4 qs[2][NS][G], ws[2][G];
    auto load_step = [&](int st, int slot) {
#pragma unroll
        for (int gk = 0; gk < G; ++gk) {
            if (MODE != 2) ws[slot][gk] = ld(w1 + 4 * (c0 + st * G + gk));
#pragma unroll
            for (int k = 0; k < NS; ++k) qs[slot][k][gk] = ld(pcrow[k] + 4 * (c0 + st * G + gk));
        }
    };
    load_step(0, 0);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
        const int cur = st & 1;
        asm volatile("" ::"s"(qs[cur][0][0][0]));   // the compiler's wait for step st sits HERE, before the next issue
        __builtin_amdgcn_sched_barrier(0);
        if (st + 1 < NST) load_step(st + 1, cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int gk = 0; gk < G; ++gk) {
            const int c = st * G + gk;
            const f32x2 p01 = {row[c][0], row[c][1]}, p23 = {row[c][2], row[c][3]};
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const f32x4 q = qs[cur][k][gk];
                const f32x2 q01 = {q[0], q[1]}, q23 = {q[2], q[3]};
                if (MODE == 0 || MODE == 3) {
                    const f32x4 ww = ws[cur][gk];
                    const f32x2 w01 = {ww[0], ww[1]}, w23 = {ww[2], ww[3]};
                    f32x2 u, v;
                    if (MODE == 3) {
                        // operands scaled by 2^-64 (w1 by 2^64): relu(p + q) IS the [0, 1] clamp of the sum, an output
                        // modifier of the packed add — one instruction for two elements where gfx950 has no packed fp32
                        // max (2 x v_max_f32 otherwise); powers of two scale exactly: same bits as the unscaled relu
                        asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(u) : "v"(p01), "s"(q01));
                        asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(v) : "v"(p23), "s"(q23));
                    } else {
                        u = p01 + q01, v = p23 + q23;               // v_pk_add_f32, scalar operand
                        u = __builtin_elementwise_max(u, (f32x2){0.f, 0.f});   // 2 x v_max_f32
                        v = __builtin_elementwise_max(v, (f32x2){0.f, 0.f});
                    }
                    s2[k] = u * w01 + s2[k];                        // v_pk_fma_f32, scalar operand
                    t2[k] = v * w23 + t2[k];
                } else {
                    s2[k] = p01 * q01 + s2[k];
                    t2[k] = p23 * q23 + t2[k];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// the slot count follows the wave's pairs np (wave-uniform); np == 0: nothing to score
template <int MODE, int G, int CB, typename Load>
__device__ __forceinline__ void tile_score(int np, const f32x4 (&row)[CB], const float* w1, const float* (&pcrow)[kTileMaxP], int c0,
                                           f32x2 (&s2)[kTileMaxP], f32x2 (&t2)[kTileMaxP], Load ld) {
    if (np > 2) tile_score_block<MODE, 4, G, CB>(row, w1, pcrow, c0, s2, t2, ld);
    else if (np == 2) tile_score_block<MODE, 2, G, CB>(row, w1, pcrow, c0, s2, t2, ld);
    else if (np == 1) tile_score_block<MODE, 1, G, CB>(row, w1, pcrow, c0, s2, t2, ld);
}

// ---- epilogue of a tile, the wave's pairs side by side (branch-free, so that the four dependency chains of DPP steps and
// exponentials interleave).  First the scores (-inf for a masked entry) and the tile maxima (wave-uniform) ...
template <int MODE>
__device__ __forceinline__ void tile_scores(const f32x2 (&s2)[kTileMaxP], const f32x2 (&t2)[kTileMaxP], bool ok, float b1,
                                            float (&sc)[kTileMaxP], float (&mx)[kTileMaxP]) {
#pragma unroll
    for (int k = 0; k < kTileMaxP; ++k) {
        const float ssum = (s2[k][0] + t2[k][0]) + (s2[k][1] + t2[k][1]);
        sc[k] = ok ? ssum + (MODE != 2 ? b1 : 0.f) : -INFINITY;
        mx[k] = sc[k];
    }
    wave_reduce_dpp_n<kTileMaxP>(mx, [](float x, float y) { return fmaxf(x, y); });
}
// ... then one pair's online-softmax step: running maximum m, per-lane partial sum l (lanes are added once, after the last tile),
// the rescale factor of what the pair has accumulated and this entry's p_e (0 unless `live`)
struct SoftmaxStep {
    float scale, pe;
};
__device__ __forceinline__ SoftmaxStep tile_softmax_step(float& m, float& l, float mx, float sc, bool live) {
    const float mnew = fmaxf(m, mx);
    const bool any = mnew != -INFINITY;            // wave-uniform; false: nothing valid so far, m, l, O stay 0
    const float scale = any ? exp_le0(m - mnew) : 1.f;       // exp(-inf) = 0 on the first valid tile
    const float pe = (any && live) ? exp_le0(sc - mnew) : 0.f;
    l = l * scale + pe;
    m = mnew;
    return {scale, pe};
}

// ---- the rating-weighted aggregation O[pair, f] = O[pair, f] scl[pair] + sum_e P[pair, e] feat[e, f] of one tile on the matrix
// cores.  Jobs: (16-pair row tile mt, 16-feature column tile nt) = (j % MT, j / MT) for j = wave, wave + NW, ..., NJ per wave at most;
// accumulator register i of a job holds pair row 16 mt + 4 g4 + i, feature 16 nt + i16  (g4 = lane >> 4, i16 = lane & 15).
template <int NW, int MT, int NJ>
__device__ __forceinline__ void tile_aggregate(f32x4 (&acc)[NJ], const float* fct, const float* Pm, const float* scl, int Fdim, int ntiles16,
                                               int wave, int g4, int i16) {
#pragma unroll
    for (int n = 0; n < NJ; ++n) {
        const int job = wave + NW * n;
        const int mt = job % MT, nt = job / MT;
        if (nt >= ntiles16) break;                  // wave-uniform
        const f32x4 s4 = *reinterpret_cast<const f32x4*>(scl + 16 * mt + 4 * g4);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[n][i] *= s4[i];
        const float* fb = fct + 16 * nt + i16;
        const float* pa = Pm + (16 * mt + i16) * kTilePS + g4;
#pragma unroll
        for (int q0 = 0; q0 < kTileEC / 4; q0 += 8) {    // 8 k-steps' operands first (16 LDS reads in flight), then their chain
            float av[8], bv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {           // A[i = pair][k = 4q + g4], B[k][j = feature]
                av[q] = pa[4 * (q0 + q)];
                bv[q] = fb[(4 * (q0 + q) + g4) * Fdim];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc[n], 0, 0, 0);
        }
    }
}
// out[pid[row], f] = O[row, f] scl[row] + bias[f] for the group's cnt pairs (scl = 1 / l by now)
template <int NW, int MT, int NJ>
__device__ __forceinline__ void tile_store_scaled(const f32x4 (&acc)[NJ], const float* scl, const int64_t* pid, int cnt, int Fdim, int ntiles16,
                                                  const float* out_bias, float* out, int64_t ldout, int wave, int g4, int i16) {
#pragma unroll
    for (int n = 0; n < NJ; ++n) {
        const int job = wave + NW * n;
        const int mt = job % MT, nt = job / MT;
        if (nt >= ntiles16) break;
        const f32x4 s4 = *reinterpret_cast<const f32x4*>(scl + 16 * mt + 4 * g4);
        const int f = 16 * nt + i16;
        const float bias = (out_bias && f < Fdim) ? out_bias[f] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 16 * mt + 4 * g4 + i;
            if (row < cnt && f < Fdim) out[pid[row] * ldout + f] = acc[n][i] * s4[i] + bias;
        }
    }
}

// ---- the merge of a pair's nsplit slice partials (m_s, l_s, -, -, O_s[..]; p0 = the first, ldpart floats apart), features 4c .. 4c+3:
//   sum_s O_s e^(m_s - M) / sum_s l_s e^(m_s - M) + bias,  M = max_s m_s   (slices in index order: deterministic, the same bits
// wherever it runs).  A pair whose slices are all empty (no rated entry: the nan_to_num case, attention_ncf.py:208-209) gets the
// bias alone.  AHEAD: up to 8 slices' (m, l) and O chunks are requested at once — a loop over a run-time count is a chain of
// dependent round trips.
template <bool AHEAD>
__device__ __forceinline__ f32x4 merge_partials(const float* p0, int nsplit, int ldpart, int c, const float* bias4) {
    float M = -INFINITY, L = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    auto weight = [&](float ms) { return (ms == -INFINITY) ? 0.f : exp_le0(ms - M); };
    if (AHEAD && nsplit <= 8) {
        f32x2 ml[8];
        f32x4 ov[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float* ps = p0 + (int64_t)(s < nsplit ? s : nsplit - 1) * ldpart;
            ml[s] = *reinterpret_cast<const f32x2*>(ps);
            ov[s] = *reinterpret_cast<const f32x4*>(ps + kPartHead + 4 * c);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) M = s < nsplit ? fmaxf(M, ml[s][0]) : M;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (s < nsplit) {
                const float w = weight(ml[s][0]);
                L += ml[s][1] * w;
                o += ov[s] * w;
            }
    } else {
        for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p0[(int64_t)s * ldpart]);
        for (int s = 0; s < nsplit; ++s) {
            const float* ps = p0 + (int64_t)s * ldpart;
            const float w = weight(ps[0]);
            L += ps[1] * w;
            o += *reinterpret_cast<const f32x4*>(ps + kPartHead + 4 * c) * w;
        }
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (bias4) bias = *reinterpret_cast<const f32x4*>(bias4 + 4 * c);
    f32x4 res;
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = o[j] * inv + bias[j];
    return res;
}

}  // namespace ncf
